"""fwav.stages without a device: every dispatching function in each variant it has (width 16, width 32, a query
table; matrix, pocketfft) names the entry point and hands over the arguments in include/fwav.h's order; the workspace
size's zero rule; the option checks; the module imports no torch; and no other module of the package names a variant
entry point."""
import ast
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "audio-compression_amd")
sys.path[:0] = [p for p in (ROOT, PKG) if p not in sys.path]

from fwav import _lib, stages  # noqa: E402

# distinct sentinels for the pointers (every one a different int) and the scalars
(SIG, TAB, POOL, EMB, EMB16, WS, RANGES, ZC, CAND, ACTIVE, NACT, TIES, RESOLVE, ROWS, SCORES, QEMB, QEMB16, NEWC, RSUB,
 STREAM) = range(1001, 1021)
N, TILE, RS, STEP, ND, K, MQ, LO, THREADS, WSB, NQ, STRIDE, MAXT, MODE, NROWS = (
    88200, 4096, 16, 4, 21027, 64, 5513, 7, 8, 4096, 5514, 3, 5512, 2, 11)
THR, FAST = 7.5e-5, 1


@pytest.fixture
def rec(monkeypatch):
    """stages.call / stages.size_call replaced by a recorder: [(name, args)]."""
    calls = []

    def call(name, *args):
        calls.append((name, args))
        return 0

    def size_call(name, *args):
        calls.append((name, args))
        return 4242

    monkeypatch.setattr(stages, "call", call)
    monkeypatch.setattr(stages, "size_call", size_call)
    return calls


def one(calls, name, args):
    """The recorder holds exactly this call, and it fills every parameter of the binding."""
    assert calls == [(name, args)]
    assert len(args) == len(_lib.SIGNATURES[name][1]), name
    calls.clear()


def test_pool_embed_and_embed_rows(rec):
    a = (SIG, N, TILE, RS, STEP, TAB, POOL, EMB, EMB16, WS, WSB, STREAM)
    stages.pool_embed(*a)
    one(rec, "fwav_pool_embed", a)
    stages.pool_embed(*a, embedding="matrix", emb_dim=16)
    one(rec, "fwav_pool_embed", a)
    stages.pool_embed(*a, embedding="pocketfft")
    one(rec, "fwav_pool_embed_exact", a)
    stages.pool_embed(*a, emb_dim=32)  # emb_dim after step
    one(rec, "fwav_pool_embed_dim", (SIG, N, TILE, RS, STEP, 32, TAB, POOL, EMB, EMB16, WS, WSB, STREAM))
    r = (RANGES, MQ, RS, TAB, QEMB, QEMB16, STREAM)
    stages.embed_rows(*r)
    one(rec, "fwav_embed_rows", r)
    stages.embed_rows(*r, embedding="pocketfft")
    one(rec, "fwav_embed_rows_exact", r)
    stages.embed_rows(RANGES, MQ, RS, TAB, QEMB, None, STREAM, embedding="matrix")
    one(rec, "fwav_embed_rows", (RANGES, MQ, RS, TAB, QEMB, None, STREAM))


def test_prune(rec):
    a = (RANGES, MQ, LO, RS, THR, FAST, EMB, ND, K, ZC, CAND, ACTIVE, NACT, STREAM)
    stages.prune(*a)
    one(rec, "fwav_prune", a)
    stages.prune(*a, emb_dim=32)  # emb_dim right after n_domains
    one(rec, "fwav_prune_dim", (RANGES, MQ, LO, RS, THR, FAST, EMB, ND, 32, K, ZC, CAND, ACTIVE, NACT, STREAM))
    stages.prune(*a, qemb=QEMB, n_query_rows=NQ)  # the query table and its rows before n_domains, in emb's place
    one(rec, "fwav_prune_q", (RANGES, MQ, LO, RS, THR, FAST, QEMB, NQ, ND, K, ZC, CAND, ACTIVE, NACT, STREAM))


def test_sim_topk(rec):
    a = (EMB, EMB16, ND, ACTIVE, NACT, MQ, LO, K, THREADS, CAND, TIES, WS, WSB, STREAM)
    stages.sim_topk(*a)
    one(rec, "fwav_sim_topk", a)
    stages.sim_topk(EMB, None, ND, ACTIVE, NACT, MQ, LO, K, THREADS, CAND, None, WS, 0, None)
    one(rec, "fwav_sim_topk", (EMB, None, ND, ACTIVE, NACT, MQ, LO, K, THREADS, CAND, None, WS, 0, None))
    stages.sim_topk(*a, emb_dim=32)
    one(rec, "fwav_sim_topk_dim", (EMB, EMB16, ND, 32, ACTIVE, NACT, MQ, LO, K, THREADS, CAND, TIES, WS, WSB, STREAM))
    stages.sim_topk(*a, query=(QEMB, QEMB16, NQ, STRIDE))
    one(rec, "fwav_sim_topk_q", (EMB, EMB16, ND, QEMB, QEMB16, NQ, STRIDE, ACTIVE, NACT, MQ, LO, K, THREADS, CAND, TIES,
                                 WS, WSB, STREAM))


def test_tie_check(rec):
    a = (RANGES, MQ, RS, CAND, K, POOL, ND, EMB, LO, THREADS, TIES, MAXT, MODE, RESOLVE, STREAM)
    stages.tie_check(*a)
    one(rec, "fwav_tie_check", a)
    stages.tie_check(*a, emb_dim=32)  # emb_dim right after emb
    one(rec, "fwav_tie_check_dim", (RANGES, MQ, RS, CAND, K, POOL, ND, EMB, 32, LO, THREADS, TIES, MAXT, MODE, RESOLVE,
                                    STREAM))
    stages.tie_check(*a, qemb=QEMB)
    one(rec, "fwav_tie_check_q", (RANGES, MQ, RS, CAND, K, POOL, ND, EMB, QEMB, LO, THREADS, TIES, MAXT, MODE, RESOLVE,
                                  STREAM))


def test_score_rows(rec):
    a = (EMB, ND, ROWS, NROWS, LO, THREADS, SCORES, STREAM)
    stages.score_rows(*a)
    one(rec, "fwav_score_rows", a)
    stages.score_rows(*a, emb_dim=32)
    one(rec, "fwav_score_rows_dim", (EMB, ND, 32, ROWS, NROWS, LO, THREADS, SCORES, STREAM))
    stages.score_rows(*a, qemb=QEMB)
    one(rec, "fwav_score_rows_q", (EMB, ND, QEMB, ROWS, NROWS, LO, THREADS, SCORES, STREAM))


def test_topk_workspace_size_and_its_zero_rule(rec):
    assert stages.topk_workspace_size(MQ, ND, K, emb_dim=16, f16=True) == 4242
    one(rec, "fwav_sim_topk_workspace_size", (MQ, ND, K))
    assert stages.topk_workspace_size(MQ, ND, 65, emb_dim=16, f16=False) == 4242
    one(rec, "fwav_sim_topk_workspace_size", (MQ, ND, 65))
    # width 16 without the fp16 table: no workspace up to K = 64, and no call
    for k in (1, 8, 64):
        assert stages.topk_workspace_size(MQ, ND, k, emb_dim=16, f16=False) == 0
        assert rec == []
    for f16 in (False, True):
        assert stages.topk_workspace_size(MQ, ND, K, emb_dim=32, f16=f16) == 4242
        one(rec, "fwav_sim_topk_dim_workspace_size", (MQ, ND, 32, K))


def test_emb16_elems_and_embed_tables_host(rec):
    assert stages.emb16_elems(ND, 16) == 4242
    one(rec, "fwav_emb16_elems", (ND,))
    assert stages.emb16_elems(ND, 32) == 4242
    one(rec, "fwav_embh_elems", (ND, 32))
    for mode, kw, size_fn, fill_fn, lead in (
            ("matrix", {}, "fwav_embed_tables_size", "fwav_embed_tables", (8,)),
            ("pocketfft", {}, "fwav_embed_tables_exact_size", "fwav_embed_tables_exact", (8,)),
            ("matrix", {"emb_dim": 32}, "fwav_embed_tables_dim_size", "fwav_embed_tables_dim", (8, 32))):
        tab = stages.embed_tables_host(8, mode, **kw)
        assert tab.dtype == np.float64 and tab.shape == (4242,)
        if mode == "pocketfft":
            assert rec.pop(0) == ("fwav_embed_exact_supported", (8,))
        assert rec == [(size_fn, lead), (fill_fn, lead + (tab.ctypes.data,))]
        assert len(lead) + 1 == len(_lib.SIGNATURES[fill_fn][1]) and len(lead) == len(_lib.SIGNATURES[size_fn][1])
        rec.clear()


def test_tie_fixup_is_the_three_launches(rec):
    tmp5, outs5 = (2001, 2002, 2003, 2004, 2005), (3001, 3002, 3003, 3004, 3005)
    stages.tie_fixup(ROWS, NROWS, NEWC, K, CAND, RANGES, RS, RSUB, tmp5, outs5, POOL, ND, 16.0, STREAM)
    assert rec == [("fwav_tie_rows_in", (ROWS, NROWS, NEWC, K, CAND, RANGES, RS, RSUB, STREAM)),
                   ("fwav_affine", (RSUB, NROWS, RS, NEWC, K, POOL, ND, 16.0, *tmp5, STREAM)),
                   ("fwav_tie_rows_out", (ROWS, NROWS, *tmp5, *outs5, STREAM))]
    for name, args in rec:
        assert len(args) == len(_lib.SIGNATURES[name][1]), name


def test_decode_loop_stops_for_the_exact_check_and_resumes(rec):
    """fwav_decode_from → (state 2) fwav_decode_exact → (state 3) resume from the host's copy of the result, the
    iterations left and the Δ pointer moved on; the loop ends when the exact check says stop (state 1)."""
    A, B, DELTAS, STATE, IDX, S, O, SYM, COPY = 5000, 6000, 7000, 8000, 11, 12, 13, 14, 9000
    states = iter([(2, 3, 1, 0), (3, 3, 1, 0),   # 3 iterations, result in b, checked: the reference goes on
                   (2, 2, 0, 0), (1, 2, 0, 0)])  # 2 more, result in a, checked: it stops
    snaps = []
    got = stages.decode(IDX, S, O, SYM, MQ, RS, POOL, ND, 8, 1e-3, 16.0, 0.5, A, B, DELTAS, STATE, WS, WSB, STREAM,
                        read_state=lambda: next(states), snapshot=lambda p: snaps.append(p) or COPY)
    assert got == (False, 5) and snaps == [B]
    head = (IDX, S, O, SYM, MQ, RS, POOL, ND)
    assert rec == [("fwav_decode_from", head + (8, 1e-3, 16.0, 0.5, None, A, B, DELTAS, STATE, WS, WSB, STREAM)),
                   ("fwav_decode_exact", (A, B, MQ * RS, 1e-3, 2, DELTAS, STATE, STREAM)),
                   ("fwav_decode_from", head + (5, 1e-3, 16.0, 0.5, COPY, A, B, DELTAS + 24, STATE, WS, WSB, STREAM)),
                   ("fwav_decode_exact", (B, A, MQ * RS, 1e-3, 1, DELTAS + 24, STATE, STREAM))]
    for name, args in rec:
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
    rec.clear()
    # no check asked for: one call; and a "go on" at the last iteration does not resume
    assert stages.decode(*head, 8, 0.0, 16.0, 0.0, A, B, DELTAS, STATE, WS, WSB, None, read_state=lambda: (0, 8, 1, 0),
                         snapshot=None) == (True, 8)
    assert [n for n, _ in rec] == ["fwav_decode_from"]
    rec.clear()
    states = iter([(2, 8, 0, 0), (3, 8, 0, 0)])
    assert stages.decode(*head, 8, 1e-3, 16.0, 0.0, A, B, DELTAS, STATE, WS, WSB, None,
                         read_state=lambda: next(states), snapshot=None) == (False, 8)
    assert [n for n, _ in rec] == ["fwav_decode_from", "fwav_decode_exact"]


def test_compact_rules():
    assert stages.compact_rows_cap(100, 7) == 7 and stages.compact_rows_cap(5, 7) == 5
    assert stages.compact_rows_cap(100, 0) == 1
    assert stages.compact_count(np.array([3, 0], np.int64)) == 3
    with pytest.raises(IndexError, match="domain index out of range"):
        stages.compact_count(np.array([3, 1], np.int64))


def test_reference_scalars():
    f32 = np.float32
    assert stages.SMOOTH_WINDOW == 5
    for thr in (1e-4, 3e-5, 0.1):
        assert stages.voiced_hi(thr) == float(f32(thr)) and stages.voiced_lo(thr) == float(f32(thr * 0.5))
        assert stages.prune_thr(thr) == float(f32(thr * 0.75))
    assert stages.is_silent(f32(9.9e-9)) and not stages.is_silent(f32(1e-8)) and stages.is_silent(0.0)
    assert not stages.is_silent(float("nan"))
    assert stages.clip32(-16.0) == 16.0 and stages.clip32(0.1) == float(f32(0.1))
    assert stages.n_domains_for(2047, 2048, 2) == 0 and stages.n_domains_for(2048, 2048, 2) == 1
    assert stages.n_domains_for(44100, 2048, 2) == 21027
    assert stages.TIE_MODES == {"numpy": 0, "numpy_sets": 1, "numpy_rows": 2, "index": -1} and stages.TIE_REC == 9


def test_checks_accept_and_refuse_what_the_layers_tests_expect():
    """The accept / refuse table of test_exact_dct.py, test_embdim_cpu.py and test_query_cpu.py, on stages itself
    (fwav_embed_exact_supported is a host call: the built library answers it)."""
    import __graft_entry__
    __graft_entry__.build()
    assert stages.check_embedding("pocketfft", 32) == "pocketfft" and stages.check_embedding("matrix", 51) == "matrix"
    for check in (stages.check_embedding, lambda m, rs: stages.embed_tables_host(rs, m)):
        with pytest.raises(ValueError, match="range size 51"):
            check("pocketfft", 51)
        with pytest.raises(ValueError, match="'matrix' or 'pocketfft'"):
            check("scipy", 8)
    assert stages.EMB_DIMS == (16, 32) and stages.check_emb_dim(16) == 16 and stages.check_emb_dim(32) == 32
    for call in (stages.check_emb_dim, lambda d, e: stages.embed_tables_host(8, e, d)):
        for bad in (8, 24, 64, 0):
            with pytest.raises(NotImplementedError, match="16 and 32"):
                call(bad, "matrix")
        with pytest.raises(ValueError, match="pocketfft.*emb_dim=32"):
            call(32, "pocketfft")
    assert stages.QUERIES == ("domain_row", "range") and stages.QUERY_RANGE_MAX_K == 64
    assert stages.check_query("domain_row", 32, 4096) == "domain_row"
    assert stages.check_query("range", 16, 64) == "range" and stages.check_query("range") == "range"
    with pytest.raises(ValueError, match="query must be"):
        stages.check_query("ranges")
    with pytest.raises(ValueError, match="emb_dim=32"):
        stages.check_query("range", emb_dim=32)
    with pytest.raises(ValueError, match="top_k"):
        stages.check_query("range", top_k=65)
    for order in stages.TIE_MODES:
        assert stages.check_tie_order(order) == order
    with pytest.raises(ValueError, match="tie_order must be 'numpy' .*'numpy_sets'.*'numpy_rows'.*'index'"):
        stages.check_tie_order("scipy")


def test_the_hosts_reexport_the_same_objects():
    pytest.importorskip("torch")
    from fwav import engine
    for name in ("EMBEDDINGS", "EMB_DIMS", "QUERIES", "QUERY_RANGE_MAX_K", "TIE_MODES", "TIE_REC", "check_embedding",
                 "check_emb_dim", "check_query", "n_domains_for", "geometry", "zero_query_candidates"):
        assert hasattr(engine, name), name
        if hasattr(stages, name):
            assert getattr(engine, name) is getattr(stages, name), name


def test_importing_stages_imports_no_torch():
    code = f"import sys; sys.path[:0] = [{PKG!r}]; import fwav.stages; assert 'torch' not in sys.modules"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]


def test_variant_entry_points_are_named_in_stages_alone():
    """A string literal that is a *_dim, *_q, *_exact or fwav_embh_* entry point occurs in _lib.py (the bindings) and
    stages.py (the table) and in no other module of the package."""
    variant = re.compile(r"^fwav_(?!debug_)\w*(_dim|_q|_exact)(_\w+)?$|^fwav_embh_\w+$")
    names = {n for n in _lib.SIGNATURES if variant.match(n)}
    assert {"fwav_sim_topk_q", "fwav_prune_dim", "fwav_pool_embed_exact", "fwav_embed_tables_exact_size",
            "fwav_sim_topk_dim_workspace_size", "fwav_embh_elems", "fwav_decode_exact", "fwav_embed_rows_exact",
            "fwav_embed_exact_supported"} <= names
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, "fwav", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value in names:
                found.setdefault(os.path.basename(path), set()).add(node.value)
    assert set(found) == {"_lib.py", "stages.py"}, {f: sorted(v) for f, v in found.items()}
    # and stages serves each of them but the two fp16-table converters, which only tests call
    assert names - found["stages.py"] == {"fwav_embh_from_emb"}
