"""The first pass's seed policy (csrc/fwav_topk_first.h seed_limit): where a floor is applied, one count
at the floor decides per query set whether the seeds' 20-step bit search runs.  The policy changes no band limit: a
query whose window holds fewer than K rows at or above the floor has a seed below the floor, which the floor replaces.

Shapes of test_gpu_centroid_qs4.py (≈ 2,100 active queries: two full 1,024-query blocks and a ragged one with empty
sets; ≈ 70,000 domains, no multiple of 32; a pruned speech-like list), in each of three forced geometries: the centroid
pre-filter with 4 and with 2 query sets per wave, and the base geometry.  Through the debug library's
fwav_debug_topk_seeds: 0 = the policy, 1 = always search (what every launch did before), 2 = never seed.

1. whole-block plan, every floor: policy and always-search give the same firing tiles, appends, compactions, level-2
   pairs and candidates, exactly; the counter of full searches reads 0 at a floor above every score, every non-empty
   set at floor 0.0, and without a floor what always-search reads;
2. every floor × plan: candidates and match tuples equal the all-f32 search's, under the policy and without any seed;
3. speech-like, the pilots' floor: every query whose seed beats the floor keeps exactly that seed under the policy."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav._lib import call, debug_library, sim_topk_layout, size_call  # noqa: E402
from test_gpu_centroid_bound import DBG_PRODUCT, _emb16, _run, _same, _search, td  # noqa: E402
from test_gpu_centroid_qs4 import SIGNALS  # noqa: E402

DBG_PROLOGUE = 64   # the prologue's counters at stats[16 .. 19], dumps from stats[32] on
DBG_SEEDS = 32768   # dump every query's seed (f32 bits) at stats[16 + position in the active list]
SEEDS_POLICY, SEEDS_ALWAYS, SEEDS_NEVER = 0, 1, 2
#: name → (fwav_debug_topk_geometry, fwav_debug_topk_cent_sets, plan_info's geometry code, queries per block)
GEOMETRIES = {"cent4": (2, 4, 3, 1024), "cent2": (2, -1, 2, 512), "base": (0, -1, 0, 256)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The signal's all-f32 reference, computed once and shared."""
    mk, tile, K, shard = SIGNALS[name]
    sig = td(mk())
    ref = _run(sig, tile, K, shard, "f32")
    cand = ref.cand.cpu().numpy().reshape(-1, K)
    na = int(ref.n_active.item())
    q = ref.active[:na].cpu().numpy().astype(np.int64)
    q = q[cand[q, -1] >= 0]
    emb = ref.emb.cpu().numpy().reshape(-1, 16).astype(np.float64)
    kth = (emb[q + shard[0]] * emb[cand[q, -1]]).sum(1)
    assert 2048 < na < 3072 and na % 32 != 0 and ref.n_domains % 32 != 0
    emb16 = _emb16(ref.emb, ref.n_domains)
    want = _search(ref.emb, None, ref.n_domains, ref.active, ref.n_active, shard[1] - shard[0], shard[0], K)
    return sig, tile, K, shard, ref, kth, emb16, want, name


@pytest.fixture(params=list(SIGNALS))
def case(request):
    return _case(request.param)


def _floors(kth):
    """Off, the pilots' own, the 5 % quantile and the median of the K-th scores, 0.0 (below every window seed that
    exists: every set searches), 0.01 above the largest K-th score (every query goes to the second pass)."""
    return [(0, 0.0), (2, 0.0), (1, float(np.quantile(kth, 0.05))), (1, float(np.median(kth))), (1, 0.0),
            (1, float(kth.max()) + 0.01)]


def _force(geo, nq, nd, plan, floor, seeds):
    g, sets, code, qb = GEOMETRIES[geo]
    call("fwav_debug_topk_geometry", g)
    call("fwav_debug_topk_cent_sets", sets)
    call("fwav_debug_topk_plan", *plan)
    call("fwav_debug_topk_floor", *floor)
    call("fwav_debug_topk_seeds", seeds)
    info = (ctypes.c_int32 * 3)()
    blocks = (ctypes.c_int64 * 3)()
    call("fwav_debug_topk_plan_info", nq, nd, info, blocks)
    assert info[0] == code and blocks[0] + blocks[1] == -(-nq // qb), (geo, list(info), list(blocks))


def _counted(ref, emb16, nq, q_offset, K, dbg, n_stats):
    """fwav_debug_sim_topk with counters: (candidates, stats, the floor's applied score or None)."""
    nd, dev = ref.n_domains, ref.emb.device
    st = torch.cuda.current_stream().cuda_stream
    wsn = size_call("fwav_sim_topk_workspace_size", nq, nd, K)
    wsk = torch.zeros(max(wsn, 16), dtype=torch.uint8, device=dev)
    cand = torch.full((nq * K,), -7, dtype=torch.int32, device=dev)
    stats = torch.zeros(n_stats, dtype=torch.int64, device=dev)
    call("fwav_debug_sim_topk", ref.emb.data_ptr(), emb16.data_ptr(), nd, ref.active.data_ptr(),
         ref.n_active.data_ptr(), nq, q_offset, K, cand.data_ptr(), wsk.data_ptr(), wsn, dbg, stats.data_ptr(), st)
    torch.cuda.synchronize()
    off = sim_topk_layout(nq, nd)["floor_key"]
    key = int(wsk[off:off + 4].cpu().numpy().view(np.uint32)[0])
    bits = np.uint32(key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff)  # key2f
    return cand.view(nq, K).cpu().numpy(), stats.cpu().numpy(), (float(bits.view(np.float32)) if key else None)


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_policy_keeps_every_limit(case, geo):
    sig, tile, K, shard, ref, kth, emb16, want, name = case
    nq, nd, na = shard[1] - shard[0], ref.n_domains, int(ref.n_active.item())
    rows = ref.active[:na].cpu().numpy().astype(np.int64)
    qb = GEOMETRIES[geo][3]
    sets_all, sets_live = -(-na // qb) * (qb // 32), -(-na // 32)  # whole blocks: every set in one item
    dbg = DBG_PRODUCT | DBG_PROLOGUE
    floors = _floors(kth)
    for floor in floors:
        got = {}
        for seeds in (SEEDS_POLICY, SEEDS_ALWAYS):
            with debug_library():
                _force(geo, nq, nd, (0, 1), floor, seeds)  # whole blocks: no timing-dependent sharing of limits
                got[seeds] = _counted(ref, emb16, nq, shard[0], K, dbg, 32)
        (c0, s0, f0), (c1, s1, f1) = got[SEEDS_POLICY], got[SEEDS_ALWAYS]
        print(f"{name} {geo} floor {floor} (applied {f0}): firing tiles {s0[1]} ({s1[1]}), appends {s0[2]} ({s1[2]}), "
              f"compactions {s0[3]} ({s1[3]}), level-2 pairs {s0[14]} ({s1[14]}), full searches {s0[18]} of "
              f"{sets_live} live sets ({s1[18]} of {sets_all} sets)")
        assert f0 == f1 and (f0 is not None) == (floor[0] != 0)
        assert [s0[i] for i in (1, 2, 3, 14)] == [s1[i] for i in (1, 2, 3, 14)], floor
        assert np.array_equal(c0, c1) and np.array_equal(c0[rows], want[rows]), floor
        assert s1[18] == sets_all, floor
        assert s0[16] > 0 and s0[17] > 0 and s0[17] <= s0[16] <= s0[6]
        if floor[0] == 0:
            assert s0[18] == s1[18]
        elif floor == floors[4]:
            assert s0[18] == sets_live
        elif floor == floors[5]:
            assert s0[18] == 0
        else:
            assert s0[18] <= sets_live


@pytest.mark.parametrize("seeds", [SEEDS_POLICY, SEEDS_NEVER])
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_every_floor_and_plan_equals_f32(case, geo, seeds):
    sig, tile, K, shard, ref, kth, emb16, want, name = case
    nq, nd = shard[1] - shard[0], ref.n_domains
    for plan in ((0, 1), (1 << 20, 3), (-1, 1)):  # whole blocks, every block in 3 table pieces, the default
        for floor in _floors(kth):
            with debug_library():
                _force(geo, nq, nd, plan, floor, seeds)
                got = _run(sig, tile, K, shard, "f16")
            _same(got, ref, (geo, seeds, plan, floor))


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_seeds_above_the_floor_survive(geo):
    sig, tile, K, shard, ref, kth, emb16, want, name = _case("speech")
    nq, nd, na = shard[1] - shard[0], ref.n_domains, int(ref.n_active.item())

    def seeds_of(floor, seeds):
        with debug_library():
            _force(geo, nq, nd, (0, 1), floor, seeds)
            _, s, f = _counted(ref, emb16, nq, shard[0], K, DBG_PRODUCT | DBG_SEEDS, 16 + nq)
        return s[16:16 + na].astype(np.uint32).view(np.float32), f

    floor = (2, 0.0)  # the pilots' own
    always, f = seeds_of(floor, SEEDS_ALWAYS)
    if not (always > f).any():  # none beats it for this signal: a floor at the median seed, so that half of them do
        floor = (1, float(np.median(always[np.isfinite(always)])))
        always, f = seeds_of(floor, SEEDS_ALWAYS)
    policy, f0 = seeds_of(floor, SEEDS_POLICY)
    beat = always > f
    print(f"speech {geo}: floor {floor} applied at {f}: {int(beat.sum())} of {na} seeds above it "
          f"(seeds {always[np.isfinite(always)].min():.3f} … {always.max():.3f})")
    assert f0 == f and beat.sum() > 0
    assert np.array_equal(policy[beat].view(np.uint32), always[beat].view(np.uint32))
    # what the policy skipped reads −∞, and only where the seed would have lost to the floor
    assert np.all((policy.view(np.uint32) == always.view(np.uint32)) | (np.isneginf(policy) & (always <= f)))
