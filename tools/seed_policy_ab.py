"""Same-process A/B of the first pass's seed policy (fwav_debug_topk_seeds: 1 = always search, the policy before
round 9; 0 = probe at the floor, then search; 2 = never seed, the ceiling of what skipping searches can win) on the
cfg2 search through libfwav_debug.so's product kernels: the modes alternated call by call, median and minimum
HIP-event times per mode, min-to-max spread of mode 1, and whether the candidates agree.
usage: [AB_NQ=330750,165375,82688,41344] [AB_ORDER=1,0,2] python tools/seed_policy_ab.py [reps]"""
import os as _os_dbg
_os_dbg.environ.setdefault("FWAV_DEBUG_LIBRARY", "1")  # the search knobs: libfwav_debug.so
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio-compression_amd")]
import numpy as np
import torch

import __graft_entry__

__graft_entry__.build()
from fwav import engine, synth  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
order = [int(m) for m in os.environ.get("AB_ORDER", "1,0,2").split(",")]
sig = torch.from_numpy(synth.noise(60.0, 44100)).cuda()
r = engine.compress_device(sig, 2048, 64, keep_intermediates=True)
torch.cuda.synchronize()
nd, nr = r.n_domains, r.n_ranges
st = torch.cuda.current_stream().cuda_stream
emb16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device="cuda")
call("fwav_emb16_from_emb", r.emb.data_ptr(), nd, emb16.data_ptr(), st)
for nq in [int(x) for x in os.environ.get("AB_NQ", str(nr)).split(",")]:
    active = torch.arange(nq, dtype=torch.int32, device="cuda")
    n_active = torch.tensor([nq], dtype=torch.int32, device="cuda")
    wsn = size_call("fwav_sim_topk_workspace_size", nq, nd, 64)
    wsk = torch.empty(wsn, dtype=torch.uint8, device="cuda")
    times = {m: [] for m in order}
    cands = {}
    for rep in range(reps + 1):
        for m in order:
            call("fwav_debug_topk_seeds", m)
            cand = torch.empty(nq * 64, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call("fwav_sim_topk", r.emb.data_ptr(), emb16.data_ptr(), nd, active.data_ptr(), n_active.data_ptr(), nq, 0,
                 64, 16, cand.data_ptr(), None, wsk.data_ptr(), wsn, st)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times[m].append(e0.elapsed_time(e1))
            cands[m] = cand
    call("fwav_debug_topk_seeds", 0)
    same = all(bool(torch.equal(cands[order[0]], cands[m])) for m in order)
    print(f"{nq} queries, order {order}: " + "; ".join(
        f"mode {m} median {np.median(times[m]):.3f} ms (min {min(times[m]):.3f}, max {max(times[m]):.3f})"
        for m in order) + f"; identical={same}", flush=True)
