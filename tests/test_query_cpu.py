"""compress_audio(query="range"), the parts that need no GPU: the keyword and its default on every public layer, the
command line, the three refusals (raised before a device is touched), the C ABI's declarations and bindings, and the
argument checks of the entry points that take a query table of their own."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_ENTRY_POINTS = ("fwav_embed_rows", "fwav_embed_rows_exact", "fwav_prune_q", "fwav_sim_topk_q", "fwav_score_rows_q",
                  "fwav_tie_check_q")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib


def test_query_keyword_and_default_on_every_layer():
    pytest.importorskip("torch")
    from fwav import api, dist, engine, hipctypes
    for fn in (engine._compress_device, api.compress_audio, api.process_file_compress):
        assert inspect.signature(fn).parameters["query"].default == "domain_row", fn
    assert engine.QUERIES == ("domain_row", "range")
    # engine.compress_device forwards its keywords to _compress_device
    assert "kwargs" in inspect.signature(engine.compress_device).parameters
    # out of scope here: the sharded and the torch-free hosts
    for fn in (dist.compress_sharded, hipctypes.compress):
        assert "query" not in inspect.signature(fn).parameters, fn
    assert inspect.signature(api.process_file_decompress).parameters["s_damping"].default == 0.0
    assert inspect.signature(api.decompress_audio).parameters["s_damping"].default == 0.0


def test_cli_parses_query_and_s_damping():
    from fwav.cli import build_parser
    P = build_parser()
    a = P.parse_args(["compress", "in.wav", "out", "--query", "range"])
    assert a.cmd == "compress" and a.query == "range" and a.tile == 1024 and a.compact is False
    assert P.parse_args(["compress", "in.wav", "out"]).query == "domain_row"
    assert P.parse_args(["compress", "in.wav", "out", "--query", "domain_row", "--compact"]).compact is True
    with pytest.raises(SystemExit):
        P.parse_args(["compress", "in.wav", "out", "--query", "pool"])
    a = P.parse_args(["decompress", "x.fwav", "--s-damping", "1e-6", "--iter", "3"])
    assert (a.cmd, a.s_damping, a.iter, a.eps) == ("decompress", 1e-6, 3, 1e-3)
    assert P.parse_args(["decompress", "x.fwav"]).s_damping == 0.0


def test_cli_hands_both_options_to_the_file_level_calls(monkeypatch):
    from fwav import cli
    seen = {}
    monkeypatch.setattr(cli, "_compress_job", lambda args: seen.setdefault("c", args))
    monkeypatch.setattr(cli, "_decompress_job", lambda args: seen.setdefault("d", args))
    cli.main(["compress", "in.wav", "outdir", "--query", "range", "--tile", "2048"])
    cli.main(["decompress", "x.fwav", "--s-damping", "0.25"])
    from fwav import api
    cp = list(inspect.signature(api.process_file_compress).parameters)
    dp = list(inspect.signature(api.process_file_decompress).parameters)
    assert dict(zip(cp, seen["c"]))["query"] == "range" and dict(zip(cp, seen["c"]))["tile"] == 2048
    assert dict(zip(dp, seen["d"]))["s_damping"] == 0.25 and len(seen["d"]) == len(dp)


def test_refusals_come_before_any_device_work(monkeypatch):
    pytest.importorskip("torch")
    from fwav import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(engine, "require_device", no_device)
    sig = np.zeros(4096, np.float32)
    with pytest.raises(ValueError, match="query must be"):
        api.compress_audio(sig, 44100, 2, query="ranges")
    with pytest.raises(ValueError, match="emb_dim=32"):
        api.compress_audio(sig, 44100, 2, query="range", emb_dim=32)
    with pytest.raises(ValueError, match="top_k"):
        api.compress_audio(sig, 44100, 2, query="range", top_k=65)
    # the engine's own check (no tensor is needed to reach it)
    assert engine.check_query("domain_row", 32, 4096) == "domain_row"  # the default path keeps every K and width
    assert engine.check_query("range", 16, 64) == "range"
    for bad in (dict(query="x"), dict(query="range", emb_dim=32), dict(query="range", top_k=65)):
        with pytest.raises(ValueError):
            engine.check_query(**bad)
    # process_file_compress returns the reference's error dict for them (it never raises)
    out = api.process_file_compress(os.path.join(ROOT, "no_such.wav"), query="range")
    assert "error" in out


def test_header_declares_and_signatures_bind_the_new_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "fwav.h")).read()
    dbg = open(os.path.join(ROOT, "include", "fwav_debug.h")).read()
    for name in Q_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in lib.SIGNATURES, name
        assert hasattr(lib.product_lib(), name) and hasattr(lib.debug_lib(), name), name
    assert re.search(r"\bint fwav_debug_sim_topk_q\(", dbg) and "fwav_debug_sim_topk_q" in lib.DEBUG_SIGNATURES
    assert not hasattr(lib.product_lib(), "fwav_debug_sim_topk_q")
    # additions only: the version callers test for is unchanged
    assert lib.product_lib().fwav_abi_version() == 5
    # the _q entry points are the plain ones plus the query table's arguments
    extra = {"fwav_prune_q": 1, "fwav_sim_topk_q": 4, "fwav_score_rows_q": 1, "fwav_tie_check_q": 1}
    for name, n in extra.items():
        assert len(lib.SIGNATURES[name][1]) == len(lib.SIGNATURES[name[:-2]][1]) + n, name
    assert lib.SIGNATURES["fwav_embed_rows"] == lib.SIGNATURES["fwav_embed_rows_exact"]


def test_q_entry_points_check_their_arguments_without_a_gpu(lib):
    L = lib.product_lib()
    p = ctypes.c_void_p(16)
    ws = L.fwav_sim_topk_workspace_size(10, 1000, 64)
    #      emb emb16 nd  qemb qemb16 nq stride active n_active max_q q_off K thr cand ties ws  bytes stream
    ok = [p, p, 1000, p, p, 2000, 4, p, p, 10, 0, 64, 1, p, None, p, ws, None]

    def rc(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.fwav_sim_topk_q(*a)

    assert L.fwav_sim_topk_q(None, *ok[1:]) == -1  # FWAV_ERR_ARG
    for pos in (3, 7, 8, 13):  # qemb, active, n_active, cand
        assert rc(**{f"a{pos}": None}) == -1, pos
    assert rc(a1=None) == -1 and b"go together" in L.fwav_last_error()  # emb16 without qemb16
    assert rc(a4=None) == -1
    assert rc(a5=0) == -2 and rc(a10=2000) == -2 and rc(a10=-1) == -2  # q_offset inside the query table
    assert rc(a6=-1) == -1 and b"seed_stride" in L.fwav_last_error()
    assert rc(a11=65) == -3 and rc(a11=0) == -3  # FWAV_ERR_K: the query-table search serves K <= 64
    assert rc(a12=0) == -1
    assert rc(a16=ws - 1) == -5 and rc(a15=None) == -5  # FWAV_ERR_WORKSPACE, sized as fwav_sim_topk's
    # more query rows than domains is legal: the checks above pass with n_query_rows = 2 x n_domains
    assert rc(a16=ws - 1, a5=10 ** 6, a10=999_999) == -5
    assert L.fwav_embed_rows(None, 10, 8, p, p, None, None) == -1
    assert L.fwav_embed_rows(p, 10, 8, None, p, None, None) == -1
    assert L.fwav_embed_rows(p, -1, 8, p, p, None, None) == -1
    assert L.fwav_embed_rows(p, 0, 8, p, p, None, None) == 0  # no rows: nothing to launch
    assert L.fwav_embed_rows_exact(p, 10, 51, p, p, None, None) == -1 and b"plan" in L.fwav_last_error()
    assert L.fwav_embed_rows_exact(p, 0, 19, p, p, None, None) == 0
    assert L.fwav_score_rows_q(p, 100, None, p, 1, 0, 1, p, None) == -1
    assert L.fwav_score_rows_q(p, 100, p, p, 0, 0, 1, p, None) == 0
    assert L.fwav_tie_check_q(p, 10, 8, p, 64, p, 100, p, None, 0, 1, p, 10, 0, p, None) == -1
    assert L.fwav_prune_q(p, 10, 0, 8, 1e-4, 1, None, 100, 50, 64, None, p, p, p, None) == -1
    assert L.fwav_prune_q(p, 10, 95, 8, 1e-4, 1, p, 100, 50, 64, None, p, p, p, None) == -2  # rows past the query table
    assert L.fwav_prune_q(p, 10, 0, 8, 1e-4, 1, p, 100, 0, 64, None, p, p, p, None) == -1  # no domains
    D = lib.debug_lib()
    assert D.fwav_debug_sim_topk_q(p, p, 1000, p, p, 2000, 4, p, p, 10, 0, 64, p, p, ws - 1, 0, None, None) in (-5,)
    assert D.fwav_debug_sim_topk_q(p, p, 1000, p, None, 2000, 4, p, p, 10, 0, 64, p, p, ws, 0, None, None) == -1
