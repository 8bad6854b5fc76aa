#!/usr/bin/env python3
"""Cost of the exact embedding (fwav_pool_embed_exact, k_embed_exact) next to the matrix one (fwav_pool_embed,
k_embed<0>) on the same input: 60 s of 44.1 kHz noise at tile 8192 (rs 32, ≈ 330,000 domains) and tile 5000 (rs 19).

Per tile: HIP events around each call (pool stage + embedding kernel, fp16 tables included), the two entry points
interleaved in one process, --reps timed launches each after --warmup; medians, their ratio, how many embedding rows
differ between the two, and the whole compress step (engine.compress_device, K = 64) in both modes, wall clock with a
device synchronisation.  One JSON line per tile.
usage: python tools/embed_exact_cost.py [--tiles 8192,5000] [--reps 30] [--warmup 5] [--seconds 60]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-compression_amd")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="8192,5000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=60.0)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from fwav import engine, synth
    from fwav._lib import call, size_call
    dev = torch.device("cuda", 0)
    sig = torch.from_numpy(synth.noise(a.seconds, 44100, seed=3)).to(dev)
    n = sig.numel()
    st = torch.cuda.current_stream(dev).cuda_stream
    for tile in (int(t) for t in a.tiles.split(",")):
        rs, step = engine.geometry(tile)
        nd = (n - tile) // step + 1
        pool = torch.empty(nd * rs, dtype=torch.float32, device=dev)
        emb16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=dev)
        wsn = size_call("fwav_pool_workspace_size", n, tile, rs, step)
        ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev)
        modes = {}
        for mode, (_, _, fn) in engine.EMBEDDINGS.items():
            modes[mode] = (fn, engine.embed_tables(rs, dev, mode),
                           torch.empty(nd * 16, dtype=torch.float32, device=dev), [])

        def launch(mode):
            fn, tab, emb, _ = modes[mode]
            call(fn, sig.data_ptr(), n, tile, rs, step, tab.data_ptr(), pool.data_ptr(), emb.data_ptr(),
                 emb16.data_ptr(), ws.data_ptr(), wsn, st)

        for i in range(a.warmup + a.reps):
            for mode in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(mode)
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    modes[mode][3].append(e0.elapsed_time(e1))
        med = {m: statistics.median(v[3]) for m, v in modes.items()}
        x, y = (modes[m][2].view(nd, 16).view(torch.int32) for m in ("matrix", "pocketfft"))
        differ = int((x != y).any(dim=1).sum())
        step_ms = {}
        for mode in modes:
            ts = []
            for i in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                engine.compress_device(sig, tile, 64, embedding=mode)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            step_ms[mode] = statistics.median(ts[1:])
        print(json.dumps({"tile": tile, "range_size": rs, "step": step, "n_domains": nd, "reps": a.reps,
                          "pool_embed_ms": {m: round(v, 4) for m, v in med.items()},
                          "pool_embed_min_ms": {m: round(min(v[3]), 4) for m, v in modes.items()},
                          "ratio_pocketfft_over_matrix": round(med["pocketfft"] / med["matrix"], 3),
                          "embedding_rows_that_differ": differ,
                          "compress_step_ms": {m: round(v, 2) for m, v in step_ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
