"""The centroid pre-filter's score-dependent bound (csrc/fwav_centroid_bound.h) in the kernel: the
debug library with the centroid geometry forced, so that about 1,100 active queries (two full 512-query blocks and a
partial one with empty sets) over tables of 20,000 … 65,000 domains (no multiple of 256 or of 32) run it.

Whatever the floor (off: cold −∞ limits, the bound's fallback; the pilots' own; one inside the K-th scores; one above
every score) and the plan (whole blocks, table pieces, query halves), the candidates and every match tuple equal the
all-f32 search's — on white noise, on speech with pruned rows and a wide spread of limits, on a periodic signal whose
bands overflow (members at +∞), and on embeddings built to stress fp16 (near-duplicates, midpoints, subnormal parts).
The bound changes which tiles are tested, never which rows pass: with the STATS counters at a fixed floor key and whole
blocks, the level-2 pairs fall against the worst-case slack's while firing tiles and appends stay equal."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import engine, synth  # noqa: E402
from fwav._lib import call, debug_library, size_call  # noqa: E402
from test_gpu_floor import _periodic  # noqa: E402
from test_gpu_parity import _adversarial_emb  # noqa: E402

GEO_CENT = 2
DBG_PRODUCT = (1 << 18) | (1 << 19)  # counters in the forced geometry, with the floor
DBG_OLD_BOUND = 2048                 # the worst-case slack alone


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _run(sig, tile, K, shard, search):
    r = engine.compress_device(sig, tile, K, energy_thresh=1e-4, keep_intermediates=True, search=search,
                               tie_order="numpy_sets", shard=shard)
    torch.cuda.synchronize()
    return r


def _same(a, b, what):
    assert np.array_equal(a.cand.cpu().numpy(), b.cand.cpu().numpy()), what
    for x, y in ((a.idx, b.idx), (a.s, b.s), (a.o, b.o), (a.sym, b.sym), (a.err, b.err)):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), what


def _is_centroid(nq, nd):
    info = (ctypes.c_int32 * 3)()
    blocks = (ctypes.c_int64 * 3)()
    call("fwav_debug_topk_plan_info", nq, nd, info, blocks)
    return info[0] == GEO_CENT


#: name → (signal, tile, K, shard of ranges): the shards hold about 1,100 searched queries
SIGNALS = {
    "noise": (lambda: synth.noise(2.0, 44100, seed=11), 2048, 64, (3000, 4100)),
    "speech": (lambda: synth.speech_like(6.0, 44100, seed=5), 4096, 17, (8000, 10300)),  # 1,073 survive the prune
    "periodic": (lambda: _periodic(24000, 96), 1024, 32, (1000, 2100)),
}


@pytest.fixture(scope="module", params=list(SIGNALS))
def case(request):
    mk, tile, K, shard = SIGNALS[request.param]
    sig = td(mk())
    ref = _run(sig, tile, K, shard, "f32")
    cand = ref.cand.cpu().numpy().reshape(-1, K)
    na = int(ref.n_active.item())
    q = ref.active[:na].cpu().numpy().astype(np.int64)
    q = q[cand[q, -1] >= 0]
    emb = ref.emb.cpu().numpy().reshape(-1, 16).astype(np.float64)
    kth = (emb[q + shard[0]] * emb[cand[q, -1]]).sum(1)
    print(f"{request.param}: {na} active queries of {shard[1] - shard[0]}, {ref.n_domains} domains, K-th scores "
          f"{kth.min():.3f} … {np.median(kth):.3f} … {kth.max():.3f}")
    assert 1024 < na < 1536 and na % 32 != 0  # two full blocks, a partial one with a partial set and empty sets
    assert 10_000 <= ref.n_domains <= 70_000 and ref.n_domains % 32 != 0
    return sig, tile, K, shard, ref, kth, request.param


def test_every_floor_and_plan_equals_f32(case):
    sig, tile, K, shard, ref, kth, name = case
    nq, nd = shard[1] - shard[0], ref.n_domains
    mid = float(np.median(kth))
    floors = [(0, 0.0), (2, 0.0), (1, mid), (1, float(np.quantile(kth, 0.05))), (1, float(kth.max()) + 0.01), (1, 10.0)]
    runs = [((-1, 1), f) for f in floors] + [((1 << 20, 2), (1, mid)), ((1 << 20, 8), (0, 0.0)), ((1 << 20, -1), (1, mid)),
                                             ((1, 3), (2, 0.0))]
    for plan, (mode, value) in runs:
        with debug_library():
            call("fwav_debug_topk_geometry", GEO_CENT)
            call("fwav_debug_topk_plan", *plan)
            call("fwav_debug_topk_floor", mode, value)
            assert _is_centroid(nq, nd)
            got = _run(sig, tile, K, shard, "f16")
        _same(got, ref, (plan, mode, value))


def _counters(emb, emb16, nd, active, n_active, nq, q_offset, K, dbg):
    st = torch.cuda.current_stream().cuda_stream
    wsn = size_call("fwav_sim_topk_workspace_size", nq, nd, K)
    wsk = torch.empty(max(wsn, 16), dtype=torch.uint8, device=emb.device)
    cand = torch.full((nq * K,), -7, dtype=torch.int32, device=emb.device)
    stats = torch.zeros(16, dtype=torch.int64, device=emb.device)
    call("fwav_debug_sim_topk", emb.data_ptr(), emb16.data_ptr(), nd, active.data_ptr(), n_active.data_ptr(), nq,
         q_offset, K, cand.data_ptr(), wsk.data_ptr(), wsn, dbg, stats.data_ptr(), st)
    torch.cuda.synchronize()
    return cand.view(nq, K).cpu().numpy(), stats.cpu().numpy()


def _search(emb, e16, nd, active, n_active, nq, q_offset, K):
    """fwav_sim_topk on its own (device order among exactly tied scores); e16 = None: the all-f32 search."""
    st = torch.cuda.current_stream().cuda_stream
    wsn = size_call("fwav_sim_topk_workspace_size", nq, nd, K)
    wsk = torch.empty(max(wsn, 16), dtype=torch.uint8, device=emb.device)
    cand = torch.full((nq * K,), -7, dtype=torch.int32, device=emb.device)
    call("fwav_sim_topk", emb.data_ptr(), e16, nd, active.data_ptr(), n_active.data_ptr(), nq, q_offset, K, 1,
         cand.data_ptr(), None, wsk.data_ptr(), wsn, st)
    torch.cuda.synchronize()
    return cand.view(nq, K).cpu().numpy()


def _emb16(emb, nd):
    e16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=emb.device)
    call("fwav_emb16_from_emb", emb.data_ptr(), nd, e16.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return e16


def _compare_bounds(emb, emb16, nd, active, n_active, nq, q_offset, K, floors, want):
    """Counters 14 (level-2 pairs), 1 (firing tiles), 2 (appends) under both bounds at fixed floor keys, whole blocks."""
    rows = active[:int(n_active.item())].cpu().numpy().astype(np.int64)
    fell = 0
    for mode, value in floors:
        with debug_library():
            call("fwav_debug_topk_geometry", GEO_CENT)
            call("fwav_debug_topk_plan", 0, 1)  # whole blocks: no limits shared between pieces (timing-dependent)
            call("fwav_debug_topk_floor", mode, value)
            assert _is_centroid(nq, nd)
            c_new, s_new = _counters(emb, emb16, nd, active, n_active, nq, q_offset, K, DBG_PRODUCT)
            c_old, s_old = _counters(emb, emb16, nd, active, n_active, nq, q_offset, K, DBG_PRODUCT | DBG_OLD_BOUND)
        print(f"floor {mode, value}: level-2 pairs {s_new[14]} (worst-case slack {s_old[14]}), firing tiles {s_new[1]} "
              f"({s_old[1]}), appends {s_new[2]} ({s_old[2]})")
        assert np.array_equal(c_new[rows], want[rows]) and np.array_equal(c_old[rows], want[rows]), (mode, value)
        assert s_old[14] > 0 and s_new[14] <= s_old[14], (mode, value, s_new[14], s_old[14])
        assert s_new[1] == s_old[1] and s_new[2] == s_old[2], (mode, value, s_new[:3], s_old[:3])
        fell += s_new[14] < s_old[14]
    return fell


def test_counters_fewer_pairs_same_tiles_and_appends(case):
    sig, tile, K, shard, ref, kth, name = case
    nq, nd = shard[1] - shard[0], ref.n_domains
    emb16 = _emb16(ref.emb, nd)
    want = _search(ref.emb, None, nd, ref.active, ref.n_active, nq, shard[0], K)
    floors = [(0, 0.0), (1, float(np.quantile(kth, 0.05))), (1, float(np.median(kth)))]
    fell = _compare_bounds(ref.emb, emb16, nd, ref.active, ref.n_active, nq, shard[0], K, floors, want)
    # (the periodic signal's domains repeat: nearly every marked pair there holds a row that passes, under either bound)
    assert fell >= 1 or name == "periodic"


@pytest.mark.parametrize("K", [64, 17])
def test_adversarial_embeddings(K):
    """Near-duplicate rows, fp16 midpoints and subnormal parts (test_hilo_band_adversarial_embeddings' table): equal
    candidates in the forced centroid geometry with and without a floor, and equal tiles and appends under both bounds."""
    nd, nq = 20_011, 1100
    dev = torch.device("cuda", 0)
    emb = td(_adversarial_emb(nd, 7).reshape(-1))
    emb16 = _emb16(emb, nd)
    act = torch.arange(nq, dtype=torch.int32, device=dev)
    n_act = torch.tensor([nq], dtype=torch.int32, device=dev)

    def search(e16):
        return _search(emb, e16, nd, act, n_act, nq, 0, K)

    want = search(None)
    assert ((want >= 0) & (want < nd)).all()
    E = emb.cpu().numpy().reshape(-1, 16).astype(np.float64)
    kth = (E[:nq] * E[want[:, -1]]).sum(1)
    floors = [(0, 0.0), (2, 0.0), (1, float(np.median(kth))), (1, 10.0)]
    for mode, value in floors:
        with debug_library():
            call("fwav_debug_topk_geometry", GEO_CENT)
            call("fwav_debug_topk_floor", mode, value)
            assert _is_centroid(nq, nd)
            assert np.array_equal(search(emb16.data_ptr()), want), (mode, value)
    _compare_bounds(emb, emb16, nd, act, n_act, nq, 0, K, [(0, 0.0), (1, float(np.median(kth)))], want)
