"""compress_audio(query="range") measured against the default query="domain_row" (DESIGN §3.8), and fit="clipped"
against the default fit="reference" (DESIGN §3.9), one JSON line each.

usage: python tools/bench_query.py search  [--config cfg2] [--reps 20] [--warmup 3] [--seconds S]
       python tools/bench_query.py quality
       python tools/bench_query.py fit     [--config cfg2] [--reps 20] [--warmup 3] [--seconds S]

search: the similarity search alone at a bench configuration's shape, by HIP events as tools/bench_embdim.py does it —
  one compress_device(query="range") call builds the domain table, the ranges' own embeddings and the active list; then
  fwav_sim_topk (queries = domain rows) and fwav_sim_topk_q (queries = the ranges' embeddings, seed_stride =
  range_size // domain_step) are launched warmup + reps times each, alternating, on one stream; the figures are
  medians.  Also fwav_embed_rows' time, and the first pass's counters from the debug library's STATS kernels in the
  product's geometry with its floor (tools/first_stats.py's): level-2 (tile, set) pairs per query set and appends per
  query — whether the centroid filter's premise (neighbouring queries are close) survives disjoint ranges.
quality: the four signals of tests/test_gpu_query_range.py::test_fit_snr_gains_at_least_3_db (K = 32) under both
  queries and both fits: the encoder's fit SNR 10·log10(Σ‖r‖² / Σ err²) over the searched ranges, and the decoded SNR
  of decompress_audio at s_damping = 0 and 1e-6 against the voiced-masked input, over the whole signal and over the
  searched ranges alone (the figure the fit SNR promises).
fit: at a bench configuration's shape, in one process: fwav_affine_fit in reference and in clipped mode on the call's
  own candidate rows, launched alternately (medians of HIP events); then whole compress_device calls under
  tie_order="numpy" with each fit — the rows ranked on the host and the wall time per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-compression_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median_ms(fns, reps, warmup):
    """Median HIP-event time of each callable, launched alternately (same process, same clocks)."""
    times = [[] for _ in fns]
    for it in range(warmup + reps):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[j].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times], [(float(min(t)), float(max(t))) for t in times]


def search(args):
    from fwav import _lib, engine, synth, ties
    from fwav._lib import call, size_call
    cfg = synth.CONFIGS[args.config]
    tile, K = cfg["tile"], cfg["top_k"]
    sig_h, _, _ = synth.make_config_signal(args.config, seconds=args.seconds, seed=0)
    dev = torch.device("cuda", 0)
    sig = torch.from_numpy(sig_h).to(dev)
    r = engine.compress_device(sig, tile, K, keep_intermediates=True, tie_order="index", query="range")
    torch.cuda.synchronize()
    nd, nq, rs, step = r.n_domains, r.n_ranges, r.range_size, r.domain_step
    na = int(r.n_active.item())
    threads = ties.blas_threads()
    st = torch.cuda.current_stream(dev).cuda_stream
    emb16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=dev)
    call("fwav_emb16_from_emb", r.emb.data_ptr(), nd, emb16.data_ptr(), st)
    qemb = torch.empty(nq * 16, dtype=torch.float32, device=dev)
    qemb16 = torch.empty(size_call("fwav_emb16_elems", nq), dtype=torch.float16, device=dev)
    tab = engine.embed_tables(rs, dev)
    cand = [torch.empty(nq * K, dtype=torch.int32, device=dev) for _ in range(2)]
    wk = size_call("fwav_sim_topk_workspace_size", nq, nd, K)
    ws = torch.empty(wk, dtype=torch.uint8, device=dev)
    stride = rs // step

    def embed():
        call("fwav_embed_rows", r.ranges.data_ptr(), nq, rs, tab.data_ptr(), qemb.data_ptr(), qemb16.data_ptr(), st)

    def dom():
        call("fwav_sim_topk", r.emb.data_ptr(), emb16.data_ptr(), nd, r.active.data_ptr(), r.n_active.data_ptr(), nq, 0,
             K, threads, cand[0].data_ptr(), None, ws.data_ptr(), wk, st)

    def rng():
        call("fwav_sim_topk_q", r.emb.data_ptr(), emb16.data_ptr(), nd, qemb.data_ptr(), qemb16.data_ptr(), nq, stride,
             r.active.data_ptr(), r.n_active.data_ptr(), nq, 0, K, threads, cand[1].data_ptr(), None, ws.data_ptr(), wk,
             st)

    embed()
    torch.cuda.synchronize()
    assert torch.equal(qemb, r.qemb)
    (t_dom, t_rng, t_emb), spread = _median_ms([dom, rng, embed], args.reps, args.warmup)
    assert torch.equal(cand[1].view(nq, K)[r.active[:na].long()], r.cand.view(nq, K)[r.active[:na].long()])
    # the first pass's counters: the debug library's STATS kernels in the product's geometry (bit 18) with its floor (19)
    D = _lib.debug_lib()
    wkd = int(D.fwav_sim_topk_workspace_size(nq, nd, K))
    wsd = torch.empty(wkd, dtype=torch.uint8, device=dev)
    counters = {}
    for name in ("domain_row", "range"):
        stats = torch.zeros(16, dtype=torch.int64, device=dev)
        if name == "domain_row":
            rc = D.fwav_debug_sim_topk(r.emb.data_ptr(), emb16.data_ptr(), nd, r.active.data_ptr(), r.n_active.data_ptr(),
                                       nq, 0, K, cand[0].data_ptr(), wsd.data_ptr(), wkd, (1 << 18) | (1 << 19),
                                       stats.data_ptr(), st)
        else:
            rc = D.fwav_debug_sim_topk_q(r.emb.data_ptr(), emb16.data_ptr(), nd, qemb.data_ptr(), qemb16.data_ptr(), nq,
                                         stride, r.active.data_ptr(), r.n_active.data_ptr(), nq, 0, K, cand[0].data_ptr(),
                                         wsd.data_ptr(), wkd, (1 << 18) | (1 << 19), stats.data_ptr(), st)
        assert rc == 0, D.fwav_last_error()
        torch.cuda.synchronize()
        sv = stats.cpu().tolist()
        qsets = max((na + 31) // 32, 1)
        tot = max(sv[6], 1)
        counters[name] = dict(level2_pairs_per_query_set=sv[14] / qsets, appends_per_query=sv[2] / max(na, 1),
                              compactions_per_query=sv[3] / max(na, 1), level1_share=sv[13] / tot,
                              barrier_share=sv[7] / tot)
    print(json.dumps(dict(what="search", config=args.config, n_queries=nq, n_active=na, n_domains=nd, top_k=K,
                          seed_stride=stride, domain_row_ms=t_dom, range_ms=t_rng, ratio=t_rng / t_dom,
                          embed_rows_ms=t_emb, min_max_ms=spread, counters=counters)))


def quality(args):
    from fwav import api, engine, synth
    dev = torch.device("cuda", 0)
    signals = {"speech_like(1.5, 44100) tile 2048": (synth.speech_like(1.5, 44100), 2048),
               "speech_like(1.5, 44100) tile 1024": (synth.speech_like(1.5, 44100), 1024),
               "sweep(1.0, 16000) tile 1024": (synth.sweep(1.0, 16000), 1024),
               "noise(1.0, 44100) tile 2048": (synth.noise(1.0, 44100), 2048)}
    for name, (sig, tile) in signals.items():
        row = dict(what="quality", signal=name)
        for q, fit in ((q, f) for q in ("domain_row", "range") for f in ("reference", "clipped")):
            r = engine.compress_device(torch.from_numpy(sig).to(dev), tile, 32, keep_intermediates=True, query=q,
                                       fit=fit)
            torch.cuda.synchronize()
            rs = r.range_size
            ranges = r.ranges.cpu().numpy().reshape(-1, rs)
            err = r.err.cpu().numpy()
            ok = np.isfinite(err)
            sig2 = (ranges[ok].astype(np.float64) ** 2).sum()
            col = row[f"{q}/{fit}"] = dict(query=q, fit=fit, mean_err=float(err[ok].mean()),
                                           fit_snr_db=float(10 * np.log10(sig2 / (err[ok].astype(np.float64) ** 2).sum())))
            masked = ranges.reshape(-1)[:len(sig)]
            for d in (0.0, 1e-6):
                rec, ran, _ = engine.decompress_device(r.idx, r.s, r.o, r.sym, r.pool, r.n_ranges, rs, s_damping=d)
                rec = rec.cpu().numpy()
                col[f"decoded_snr_db_s_damping_{d:g}"] = float(api.compute_snr(masked, rec[:len(sig)]))
                noise = ((rec.reshape(-1, rs)[ok].astype(np.float64) - ranges[ok]) ** 2).sum()
                col[f"decoded_searched_snr_db_s_damping_{d:g}"] = float(10 * np.log10(sig2 / noise))
                col[f"iterations_s_damping_{d:g}"] = ran
        row["n_ranges"], row["n_domains"] = r.n_ranges, r.n_domains
        print(json.dumps(row), flush=True)


def fit(args):
    import time

    from fwav import engine, stages, synth
    cfg = synth.CONFIGS[args.config]
    tile, K = cfg["tile"], cfg["top_k"]
    sig_h, _, _ = synth.make_config_signal(args.config, seconds=args.seconds, seed=0)
    dev = torch.device("cuda", 0)
    sig = torch.from_numpy(sig_h).to(dev)
    r = engine.compress_device(sig, tile, K, keep_intermediates=True)
    torch.cuda.synchronize()
    nd, nq, rs = r.n_domains, r.n_ranges, r.range_size
    st = torch.cuda.current_stream(dev).cuda_stream
    outs = {f: [torch.empty(nq, dtype=t.dtype, device=dev) for t in (r.idx, r.s, r.o, r.sym, r.err)]
            for f in stages.FITS}

    def solve(f):
        return lambda: stages.affine(r.ranges.data_ptr(), nq, rs, r.cand.data_ptr(), K, r.pool.data_ptr(), nd, 16.0,
                                     [t.data_ptr() for t in outs[f]], st, fit=f)

    (t_ref, t_clip), spread = _median_ms([solve("reference"), solve("clipped")], args.reps, args.warmup)
    changed = int(((outs["reference"][0] != outs["clipped"][0]) | (outs["reference"][3] != outs["clipped"][3])).sum())
    print(json.dumps(dict(what="fit affine", config=args.config, n_ranges=nq, n_domains=nd, top_k=K, range_size=rs,
                          reference_ms=t_ref, clipped_ms=t_clip, ratio=t_clip / t_ref, min_max_ms=spread,
                          matches_changed=changed)), flush=True)
    for f in stages.FITS:
        wall = []
        for it in range(args.warmup + max(args.reps // 4, 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = engine.compress_device(sig, tile, K, tie_order="numpy", fit=f)
            torch.cuda.synchronize()
            if it >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="fit ties", config=args.config, fit=f, tie_order="numpy", rows_with_exact_ties=x.n_ties,
                              rows_ranked_by_numpy=x.n_resolved, call_ms_median=float(np.median(wall)),
                              call_ms_min_max=(float(min(wall)), float(max(wall))))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("search", "quality", "fit"))
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=None, help="override the signal length")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    {"search": search, "quality": quality, "fit": fit}[args.what](args)


if __name__ == "__main__":
    main()
