"""Time the similarity search alone at a bench configuration's shape for emb_dim = 32 (fwav_sim_topk_dim), or for
emb_dim = 16 (fwav_sim_topk) with the same method, and print one JSON line.

usage: python tools/bench_embdim.py [--emb-dim 32] [--config cfg2] [--top-k K] [--reps 20] [--warmup 3] [--seconds S]

The signal, tile and K are bench.py's (fwav.synth.CONFIGS); one compress_device call builds the embedding table, the
active list and the fp16 table, then the search is launched `warmup` + `reps` times on one stream, each launch between
two HIP events; the figure is the median.  `mfma_frac` is the ALGORITHMIC work of the scores, 2·queries·domains·emb_dim
flop, over the time and the dense fp16 MFMA peak (bench.py's constant) — an effective rate, as bench.py's roofline.
Outputs are not compared here (tests/test_gpu_embdim.py does that)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-compression_amd")]

import torch  # noqa: E402

F16_MFMA_PEAK_TF = 2516.6  # bench.py: v_mfma_f32_32x32x16_f16, 32 cycles/SIMD, 1024 SIMDs, 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emb-dim", type=int, choices=(16, 32), default=32)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=None, help="override the signal length")
    ap.add_argument("--top-k", type=int, default=None,
                    help="K instead of the configuration's (K = 1 keeps almost nothing: the streaming part alone)")
    args = ap.parse_args()
    from fwav import _lib
    try:
        _lib.product_lib()
    except _lib.FwavError:
        import __graft_entry__
        __graft_entry__.build()
    from fwav import engine, synth, ties
    from fwav._lib import call, size_call

    dim = args.emb_dim
    cfg = synth.CONFIGS[args.config]
    tile, K = cfg["tile"], (cfg["top_k"] if args.top_k is None else args.top_k)
    sig_h, _, _ = synth.make_config_signal(args.config, seconds=args.seconds, seed=0)
    dev = torch.device("cuda", 0)
    sig = torch.from_numpy(sig_h).to(dev)
    r = engine.compress_device(sig, tile, K, emb_dim=dim, keep_intermediates=True, tie_order="index")
    torch.cuda.synchronize()
    nd, nq = r.n_domains, r.n_ranges
    n_active = int(r.n_active.item())
    threads = ties.blas_threads()
    st = torch.cuda.current_stream(dev).cuda_stream
    cand = torch.empty(nq * K, dtype=torch.int32, device=dev)
    if dim == 16:
        tab = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=dev)
        call("fwav_emb16_from_emb", r.emb.data_ptr(), nd, tab.data_ptr(), st)
        wk = size_call("fwav_sim_topk_workspace_size", nq, nd, K)
    else:
        tab = torch.empty(size_call("fwav_embh_elems", nd, dim), dtype=torch.float16, device=dev)
        call("fwav_embh_from_emb", r.emb.data_ptr(), nd, dim, tab.data_ptr(), st)
        wk = size_call("fwav_sim_topk_dim_workspace_size", nq, nd, dim, K)
    ws = torch.empty(max(wk, 16), dtype=torch.uint8, device=dev)

    def launch():
        if dim == 16:
            call("fwav_sim_topk", r.emb.data_ptr(), tab.data_ptr(), nd, r.active.data_ptr(), r.n_active.data_ptr(), nq,
                 0, K, threads, cand.data_ptr(), None, ws.data_ptr(), wk, st)
        else:
            call("fwav_sim_topk_dim", r.emb.data_ptr(), tab.data_ptr(), nd, dim, r.active.data_ptr(),
                 r.n_active.data_ptr(), nq, 0, K, threads, cand.data_ptr(), None, ws.data_ptr(), wk, st)

    ms = []
    for i in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            ms.append(a.elapsed_time(b))
    ms.sort()
    med = ms[len(ms) // 2]
    same = bool(torch.equal(cand.view(nq, K), r.cand.view(nq, K)))
    flop = 2.0 * n_active * nd * dim
    print(json.dumps({"tool": "bench_embdim", "config": args.config, "emb_dim": dim, "queries": nq, "active": n_active,
                      "domains": nd, "top_k": K, "blas_threads": threads, "reps": len(ms), "search_ms_median": med,
                      "search_ms_min": ms[0], "search_ms_max": ms[-1], "algorithmic_flop": flop,
                      "mfma_tflops": flop / (med * 1e-3) / 1e12,
                      "mfma_frac": flop / (med * 1e-3) / 1e12 / F16_MFMA_PEAK_TF,
                      "same_candidates_as_compress_device": same}))


if __name__ == "__main__":
    main()
