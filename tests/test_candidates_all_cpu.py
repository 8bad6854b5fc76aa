"""compress_audio(candidates="all") without a device: the keyword's defaults and checks, the CLI, fwav_affine_all's
C ABI (declared, bound, argument checks, launch geometry) and the numpy restatement's own property — the exhaustive
minimum runs over a superset of the K = 32 path's slots with the same per-slot arithmetic, so its error is never
larger (no tolerance) and is smaller somewhere."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fit_all as FA
import fit_clipped as FC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fwav_affine_all_workspace_size", "fwav_affine_all_tile_rows", "fwav_affine_all_slices",
                "fwav_affine_all")
OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib


def test_defaults_and_the_hosts_left_out():
    pytest.importorskip("torch")
    from fwav import api, dist, engine, hipctypes, stages
    assert stages.CANDIDATES == ("embedding", "all") and engine.CANDIDATES is stages.CANDIDATES
    assert engine.check_candidates is stages.check_candidates
    for fn in (api.compress_audio, api.process_file_compress, engine._compress_device):
        assert inspect.signature(fn).parameters["candidates"].default == "embedding", fn
    assert list(inspect.signature(api.process_file_compress).parameters)[-1] == "candidates"
    for fn in (dist.compress_sharded, hipctypes.compress):
        assert "candidates" not in inspect.signature(fn).parameters, fn
    for c in stages.CANDIDATES:
        assert stages.check_candidates(c) == c
    for bad in ("every", "", None, 1, "ALL"):
        with pytest.raises(ValueError, match="candidates must be 'embedding' or 'all', not"):
            stages.check_candidates(bad)


def test_refusals_come_before_any_device_work(monkeypatch):
    pytest.importorskip("torch")
    from fwav import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(engine, "require_device", no_device)
    with pytest.raises(ValueError, match="candidates must be"):
        api.compress_audio(np.zeros(4096, F32), 44100, 2, candidates="every")
    # the options that "all" leaves unused are validated as today
    with pytest.raises(ValueError, match="query must be"):
        api.compress_audio(np.zeros(4096, F32), 44100, 2, candidates="all", query="tile")
    with pytest.raises(ValueError, match="fit must be"):
        api.compress_audio(np.zeros(4096, F32), 44100, 2, candidates="all", fit="clip")
    with pytest.raises(NotImplementedError):
        api.compress_audio(np.zeros(4096, F32), 44100, 2, candidates="all", emb_dim=24)
    assert "error" in api.process_file_compress("/nonexistent/in.wav", candidates="all")


def test_cli_hands_candidates_to_the_file_level_call(monkeypatch):
    from fwav import api, cli
    P = cli.build_parser()
    assert P.parse_args(["compress", "in.wav", "out"]).candidates == "embedding"
    assert P.parse_args(["compress", "in.wav", "out", "--candidates", "all"]).candidates == "all"
    with pytest.raises(SystemExit):
        P.parse_args(["compress", "in.wav", "out", "--candidates", "every"])
    seen = {}
    monkeypatch.setattr(cli, "_compress_job", lambda args: seen.setdefault("c", args))
    cli.main(["compress", "in.wav", "outdir", "--candidates", "all", "--fit", "clipped"])
    cp = list(inspect.signature(api.process_file_compress).parameters)
    assert len(seen["c"]) == len(cp)
    assert seen["c"][cp.index("candidates")] == "all" and seen["c"][cp.index("fit")] == "clipped"
    seen.clear()
    cli.main(["compress", "in.wav", "outdir"])
    assert seen["c"][cp.index("candidates")] == "embedding"


def test_header_declares_and_lib_binds_the_entry_points(lib):
    text = open(os.path.join(ROOT, "include", "fwav.h")).read()
    L = lib.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(size_t|int)\s+" + name + r"\s*\(", text), name
        assert name in lib.SIGNATURES and hasattr(L, name), name
    assert len(lib.SIGNATURES["fwav_affine_all"][1]) == 18
    assert L.fwav_abi_version() == 5  # an addition only


def test_error_codes_without_gpu(lib):
    L = lib.lib()
    p = ctypes.c_void_p(4096)

    def run(ranges=p, n_ranges=10, rs=8, active=None, n_active=None, max_q=10, pool=p, nd=100, outs=(p,) * 5, fit=1,
            ws=None, ws_bytes=0):
        return L.fwav_affine_all(ranges, n_ranges, rs, active, n_active, max_q, pool, nd, 16.0, *outs, fit, ws, ws_bytes,
                                 None)

    for fit in (2, -1, 7):  # before the pointer checks, as fwav_affine_fit
        assert run(ranges=None, pool=None, outs=(None,) * 5, fit=fit) == ERR_ARG and b"fit" in L.fwav_last_error(), fit
    for fit in (0, 1):
        assert run(ranges=None, fit=fit) == ERR_ARG and b"null" in L.fwav_last_error()
        assert run(pool=None, fit=fit) == ERR_ARG
        assert run(outs=(p, p, None, p, p), fit=fit) == ERR_ARG
        assert run(active=p, n_active=None, fit=fit) == ERR_ARG      # a list without its count
        assert run(nd=0, fit=fit) == ERR_SHAPE
        assert run(nd=1 << 30, fit=fit) == ERR_SHAPE                 # keys are 32 bits
        assert run(rs=0, fit=fit) == ERR_SHAPE
        assert run(max_q=9, fit=fit) == ERR_SHAPE                    # every row listed, fewer positions than rows
        # a split launch without its workspace, and with one byte too few
        need = L.fwav_affine_all_workspace_size(8, 70000, 8)
        assert need > 0
        assert run(n_ranges=8, max_q=8, nd=70000, fit=fit) == ERR_WORKSPACE
        assert run(n_ranges=8, max_q=8, nd=70000, ws=p, ws_bytes=need - 1, fit=fit) == ERR_WORKSPACE
        assert run(n_ranges=0, max_q=0, fit=fit) == OK               # nothing to do: no launch


def test_launch_geometry(lib):
    L = lib.lib()
    for rs in (4, 5, 8, 16, 19, 32):
        T = L.fwav_affine_all_tile_rows(rs)
        assert T > 0, rs
        for mq, nd in ((1, 1), (8, 70000), (257, 4096), (330750, 1321977), (1, T), (1, 4 * T + 1)):
            s = L.fwav_affine_all_slices(mq, nd, rs)
            assert 1 <= s <= max(1, -(-nd // T)), (rs, mq, nd, s)
            ws = L.fwav_affine_all_workspace_size(mq, nd, rs)
            assert (ws == 0) == (s == 1) and ws >= (s > 1) * s * mq * 17, (rs, mq, nd, s, ws)
    assert L.fwav_affine_all_slices(8, 70000, 8) > 1
    assert L.fwav_affine_all_slices(8, 70000, 19) > 1
    assert L.fwav_affine_all_slices(330750, 1321977, 4) == 1  # enough ranges: no split, no workspace


@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
def test_exhaustive_error_never_exceeds_the_candidate_paths(fit):
    """speech_like(0.5, 44100) at tile 1024: over the searched rows the exhaustive err is ≤ the K = 32 path's err with
    no tolerance — the minimum over a superset of slots with the same per-slot arithmetic, in the order that puts the
    smaller error first — and strictly smaller on some row."""
    c = FC.restated("speech", 1024, "domain_row")
    a = FA.restate_compress_all(c["sig"], 1024, fit)
    assert np.array_equal(a["ranges"].view(np.uint32), c["ranges"].view(np.uint32))
    assert np.array_equal(a["pool"].view(np.uint32), c["pool"].view(np.uint32))
    e_k = np.asarray((c["m"], c["mc"])[fit][4])
    e_all = a["m"][4]
    searched = ~a["pruned"]
    assert searched.any() and np.array_equal(np.isfinite(e_k), searched) and np.array_equal(np.isfinite(e_all), searched)
    assert np.all(e_all[searched] <= e_k[searched])
    n_less = int((e_all[searched] < e_k[searched]).sum())
    print(f"fit {FA.FIT_NAMES[fit]}: exhaustive err < K=32 err on {n_less} of {int(searched.sum())} searched rows; fit SNR "
          f"{FC.snr_db(a['ranges'], e_all, searched):.2f} dB against {FC.snr_db(c['ranges'], e_k, searched):.2f} dB")
    assert n_less >= 1
    # the pruned rows' tuple is the all-−1 row's: domain 0, unmirrored, err +inf
    gone = a["pruned"]
    assert np.all(a["m"][0][gone] == 0) and np.all(a["m"][3][gone] == 0) and np.all(np.isinf(e_all[gone]))
