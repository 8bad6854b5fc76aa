"""The centroid pre-filter with four query sets per wave (one centroid per 4 consecutive queries, 1,024 queries per
workgroup, the per-set buffer state kept in LDS between a set's level-2 pairs), forced through the debug
library (geometry 2 with fwav_debug_topk_cent_sets(4)) at small shapes: about 2,100 active queries — two full
1,024-query blocks and a ragged third whose last quad has fewer than 4 members and whose later sets have none — over
about 70,000 domains (no multiple of 256 or of 32).

Whatever the floor (off: cold −∞ limits; the pilots' own; one above every score, which sends every query to the second
pass) and the plan (whole blocks, every block in 3 table pieces, the default), the candidates and every match tuple
equal the all-f32 search's exactly — on white noise, and on speech-like input whose pruned active list has gaps, so
that a quad's members lie far apart, its radii are large and the filter falls back to the worst-case slack.  The
score-dependent bound changes which tiles are tested, never which rows pass: against the worst-case slack alone (dbg
2048) the firing tiles and appends are equal and the level-2 pairs no more."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import synth  # noqa: E402
from fwav._lib import call, debug_library  # noqa: E402
from test_gpu_centroid_bound import DBG_OLD_BOUND, DBG_PRODUCT, _counters, _emb16, _run, _same, _search, td  # noqa: E402

GEO_CENT = 2
GEO_CODE_1024 = 3  # what plan_info reports for 1,024-query centroid blocks
QB = 1024

#: name → (signal, tile, K, shard of ranges)
SIGNALS = {
    "noise": (lambda: synth.noise(3.2, 44100, seed=11), 2048, 64, (3000, 5102)),
    "speech": (lambda: synth.speech_like(6.0, 44100, seed=5), 4096, 17, (6000, 10600)),  # ≈ 2,220 survive the prune
}


def _is_geo4(nq, nd):
    info = (ctypes.c_int32 * 3)()
    blocks = (ctypes.c_int64 * 3)()
    call("fwav_debug_topk_plan_info", nq, nd, info, blocks)
    return info[0] == GEO_CODE_1024 and blocks[0] + blocks[1] == -(-nq // QB)


@pytest.fixture(scope="module", params=list(SIGNALS))
def case(request):
    mk, tile, K, shard = SIGNALS[request.param]
    sig = td(mk())
    ref = _run(sig, tile, K, shard, "f32")
    cand = ref.cand.cpu().numpy().reshape(-1, K)
    na = int(ref.n_active.item())
    q = ref.active[:na].cpu().numpy().astype(np.int64)
    gaps = int((np.diff(np.sort(q)) > 1).sum())
    q = q[cand[q, -1] >= 0]
    emb = ref.emb.cpu().numpy().reshape(-1, 16).astype(np.float64)
    kth = (emb[q + shard[0]] * emb[cand[q, -1]]).sum(1)
    print(f"{request.param}: {na} active queries of {shard[1] - shard[0]} ({gaps} gaps), {ref.n_domains} domains, K-th "
          f"scores {kth.min():.3f} … {np.median(kth):.3f} … {kth.max():.3f}")
    assert 2 * QB < na < 3 * QB  # two full blocks and a ragged one, some of whose sets have no members
    assert ref.n_domains % 32 != 0
    if request.param == "noise":
        assert na % 4 != 0 and 60_000 <= ref.n_domains <= 80_000  # the last quad has fewer than 4 members
    else:
        assert gaps > 10  # a pruned list: quads across gaps
    return sig, tile, K, shard, ref, kth, request.param


def test_every_floor_and_plan_equals_f32(case):
    sig, tile, K, shard, ref, kth, name = case
    nq, nd = shard[1] - shard[0], ref.n_domains
    floors = [(0, 0.0), (2, 0.0), (1, float(kth.max()) + 0.01)]
    runs = [(plan, f) for plan in ((0, 1), (1 << 20, 3)) for f in floors] + [((-1, 1), (2, 0.0))]
    for plan, (mode, value) in runs:
        with debug_library():
            call("fwav_debug_topk_geometry", GEO_CENT)
            call("fwav_debug_topk_cent_sets", 4)
            call("fwav_debug_topk_plan", *plan)
            call("fwav_debug_topk_floor", mode, value)
            assert _is_geo4(nq, nd)
            got = _run(sig, tile, K, shard, "f16")
        _same(got, ref, (plan, mode, value))


def test_counters_against_the_worst_case_slack(case):
    """Counters 14 (level-2 pairs), 1 (firing tiles), 2 (appends) under both bounds at fixed floor keys, whole blocks
    (no limits shared between pieces: those are timing-dependent)."""
    sig, tile, K, shard, ref, kth, name = case
    nq, nd = shard[1] - shard[0], ref.n_domains
    emb16 = _emb16(ref.emb, nd)
    want = _search(ref.emb, None, nd, ref.active, ref.n_active, nq, shard[0], K)
    rows = ref.active[:int(ref.n_active.item())].cpu().numpy().astype(np.int64)
    fell = 0
    for mode, value in [(0, 0.0), (1, float(np.quantile(kth, 0.05))), (1, float(np.median(kth)))]:
        with debug_library():
            call("fwav_debug_topk_geometry", GEO_CENT)
            call("fwav_debug_topk_cent_sets", 4)
            call("fwav_debug_topk_plan", 0, 1)
            call("fwav_debug_topk_floor", mode, value)
            assert _is_geo4(nq, nd)
            c_new, s_new = _counters(ref.emb, emb16, nd, ref.active, ref.n_active, nq, shard[0], K, DBG_PRODUCT)
            c_old, s_old = _counters(ref.emb, emb16, nd, ref.active, ref.n_active, nq, shard[0], K,
                                     DBG_PRODUCT | DBG_OLD_BOUND)
        print(f"floor {mode, value}: level-2 pairs {s_new[14]} (worst-case slack {s_old[14]}), firing tiles {s_new[1]} "
              f"({s_old[1]}), appends {s_new[2]} ({s_old[2]})")
        assert np.array_equal(c_new[rows], want[rows]) and np.array_equal(c_old[rows], want[rows]), (mode, value)
        assert s_old[14] > 0 and s_new[14] <= s_old[14], (mode, value, s_new[14], s_old[14])
        assert s_new[1] == s_old[1] and s_new[2] == s_old[2], (mode, value, s_new[:3], s_old[:3])
        fell += s_new[14] < s_old[14]
    assert fell >= 1
