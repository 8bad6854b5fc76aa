"""Cost of the compact option at cfg2 (60 s of 44.1 kHz noise, tile 2048, top-K 64): fwav_compact_domains on the real
match set, api.compress_audio with and without compact=True in one process (alternating), and the .fwav files' sizes
and save / load times.  Prints one JSON line (DESIGN.md §3.7 quotes it).  tools only: not part of bench.py.

  python tools/compact_bench.py [--calls 20] [--api-calls 12] [--seconds 60]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-compression_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

HBM_PEAK = 8e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--api-calls", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=60.0)
    a = ap.parse_args()
    __graft_entry__.build()
    from fwav import api, engine, synth
    from fwav._lib import call, size_call
    from fwav.fwavio import load_compressed, save_compressed

    dev = torch.device("cuda", 0)
    sig = synth.noise(a.seconds, 44100)
    res = engine.compress_device(torch.from_numpy(sig).to(dev), 2048, 64)
    torch.cuda.synchronize()
    nr, nd, rs = res.n_ranges, res.n_domains, res.range_size
    cap = min(nd, nr)
    iout = torch.empty(nr, dtype=torch.int32, device=dev)
    pout = torch.empty(cap * rs, dtype=torch.float32, device=dev)
    kept = torch.empty(cap, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    wsn = size_call("fwav_compact_workspace_size", nd, nr)
    ws = torch.empty(wsn, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ms = []
    for i in range(5 + a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call("fwav_compact_domains", res.idx.data_ptr(), nr, res.pool.data_ptr(), nd, rs, iout.data_ptr(),
             pout.data_ptr(), kept.data_ptr(), counts.data_ptr(), ws.data_ptr(), wsn, st)
        e1.record()
        e1.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    m = int(counts.cpu()[0])
    # each launch by HIP events (the debug library's entry point records one between the launches)
    import ctypes
    from fwav import _lib
    stage = (ctypes.c_float * 6)()
    per = []
    with _lib.debug_library():
        for i in range(5 + a.calls):
            call("fwav_debug_compact_stage_ms", res.idx.data_ptr(), nr, res.pool.data_ptr(), nd, rs, iout.data_ptr(),
                 pout.data_ptr(), kept.data_ptr(), counts.data_ptr(), ws.data_ptr(), wsn, st,
                 ctypes.addressof(stage))
            if i >= 5:
                per.append(list(stage))
    names = ("zero", "mark", "count", "scan", "gather", "renumber")
    launch_us = {n: round(1e3 * statistics.median(p[j] for p in per), 2) for j, n in enumerate(names)}
    words = -(-nd // 64)
    # idx read twice and written once, the bitmap written once and read twice, the prefixes written and read once,
    # the kept rows read and written
    moved = 4 * nr * 2 + 4 * nr + 8 * words * 3 + 4 * words * 2 + 2 * 4 * rs * m
    k_ms = statistics.median(ms)
    out = dict(n_ranges=nr, n_domains=nd, range_size=rs, m=m, kernel_call_ms=round(k_ms, 4),
               kernel_call_ms_min_max=[round(min(ms), 4), round(max(ms), 4)], launch_us=launch_us, bytes_moved=moved,
               hbm_fraction=round(moved / (k_ms * 1e-3) / HBM_PEAK, 5))

    if a.api_calls <= 0:  # the kernel alone (a profiler run)
        print(json.dumps(out))
        return
    t = {False: [], True: []}
    last = {}
    for i in range(2 + a.api_calls):
        for c in ((False, True) if i % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[c] = api.compress_audio(sig, 44100, 4, tile_size=2048, top_k=64, device=dev, compact=c)
            if i >= 2:
                t[c].append(1e3 * (time.perf_counter() - t0))
    out.update(api_full_ms=round(statistics.median(t[False]), 3), api_compact_ms=round(statistics.median(t[True]), 3),
               api_full_ms_min_max=[round(min(t[False]), 3), round(max(t[False]), 3)],
               api_compact_ms_min_max=[round(min(t[True]), 3), round(max(t[True]), 3)])
    with tempfile.TemporaryDirectory() as d:
        for c, name in ((False, "full"), (True, "compact")):
            r = last[c]
            path = os.path.join(d, name + ".fwav")
            sv, ld = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                save_compressed(path, r[0], r[1], r[3], 44100, 4, r[4], r[5], r[6], r[7])
                t1 = time.perf_counter()
                back = load_compressed(path)
                t2 = time.perf_counter()
                sv.append(1e3 * (t1 - t0))
                ld.append(1e3 * (t2 - t1))
            assert np.array_equal(back[1].view(np.uint32), r[1].view(np.uint32))
            out[f"fwav_{name}_bytes"] = os.path.getsize(path)
            out[f"fwav_{name}_save_ms"] = round(statistics.median(sv), 2)
            out[f"fwav_{name}_load_ms"] = round(statistics.median(ld), 2)
    out["input_f32_bytes"] = int(sig.nbytes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
