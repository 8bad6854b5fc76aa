"""compress_audio(candidates="all") measured: fwav_affine_all's time at a bench configuration's shape and
at a short speech-like one, beside the default search's, and the quality columns of the README's table.

usage: python tools/bench_affine_all.py time    [--config cfg2 | --speech 1.5] [--fit clipped] [--reps 3] [--warmup 1]
       python tools/bench_affine_all.py quality
       python tools/bench_affine_all.py run     [--out profiles/affine_all]

time: one default compress_device call builds the ranges and the pool and times the default search (its "sim_topk" and
  "affine" events); then fwav_prune_energy's list and fwav_affine_all are launched warmup + reps times on one stream,
  each between two HIP events, over the listed ranges (the product's call) and, with --every, over every range (the
  full n_ranges × n_domains rectangle).  One JSON line: medians, min/max, the pairs per second and the share of the
  instruction floor (FLOOR_VALU wave-instructions per pair, counted from the built kernel's inner loop: DESIGN §3.10).
quality: the four signals of tools/bench_query.py's table with candidates="all", fit="clipped": the fit SNR
  10·log10(Σ‖r‖² / Σ err²) over the searched ranges and the decoded SNR of decompress_audio(s_damping=1e-6) over the
  same ranges against the voiced-masked input; beside them the default candidates under the same fit.
run: every step above as a process of its own under its own time limit, chained with &&, logs under --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-compression_amd")]

#: VALU instructions per (range, domain) pair — both orientations — on the inner loop's common path (no √), by range
#: size: counted in the disassembly of k_all<RS, clipped>; a wave64 instruction issues in 4 cycles
FLOOR_VALU = {4: 77, 8: 127, 16: 209}
SIMDS, CLOCK_HZ = 1024, 2.4e9


def _events_ms(ev, name):
    a, b = ev[name][0], ev[name][-1]
    return a.elapsed_time(b)


def time_shape(args):
    import numpy as np
    import torch

    from fwav import engine, stages, synth
    dev = torch.device("cuda", 0)
    if args.speech is not None:
        sig_h, tile, K, label = synth.speech_like(args.speech, 44100), 1024, 32, f"speech_like({args.speech}, 44100)"
    else:
        cfg = synth.CONFIGS[args.config]
        tile, K, label = cfg["tile"], cfg["top_k"], args.config
        sig_h, _, _ = synth.make_config_signal(args.config, seed=0)
    sig = torch.from_numpy(sig_h).to(dev)
    engine.compress_device(sig, tile, K, tie_order="index")  # warm-up of the default path
    torch.cuda.synchronize()
    ev = {}
    r = engine.compress_device(sig, tile, K, tie_order="index", keep_intermediates=True, events=ev)
    torch.cuda.synchronize()
    nd, nr, rs = r.n_domains, r.n_ranges, r.range_size
    st = torch.cuda.current_stream(dev).cuda_stream
    active = torch.empty(nr, dtype=torch.int32, device=dev)
    n_active = torch.zeros(1, dtype=torch.int32, device=dev)
    stages.prune_energy(r.ranges.data_ptr(), nr, rs, stages.prune_thr(1e-4), 1, active.data_ptr(), n_active.data_ptr(), st)
    listed = int(n_active.item())
    outs = [torch.empty(nr, dtype=t.dtype, device=dev) for t in (r.idx, r.s, r.o, r.sym, r.err)]
    wn = stages.affine_all_workspace_size(nr, nd, rs)
    ws = torch.empty(max(wn, 16), dtype=torch.uint8, device=dev)

    def solve(every):
        stages.affine_all(r.ranges.data_ptr(), nr, rs, None if every else active.data_ptr(),
                          None if every else n_active.data_ptr(), nr, r.pool.data_ptr(), nd, 16.0,
                          [t.data_ptr() for t in outs], ws.data_ptr(), wn, st, fit=args.fit)

    out = dict(what="affine_all", shape=label, tile=tile, range_size=rs, n_ranges=nr, n_listed=listed, n_domains=nd,
               fit=args.fit, slices=int(engine.size_call("fwav_affine_all_slices", nr, nd, rs)),
               default_search_ms=_events_ms(ev, "sim_topk"), default_affine_ms=_events_ms(ev, "affine"))
    for every in ((False, True) if args.every else (False,)):
        ms = []
        for it in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solve(every)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        pairs = (nr if every else listed) * nd
        med = float(np.median(ms))
        row = dict(ms_median=med, ms_min_max=(float(min(ms)), float(max(ms))), pairs=pairs,
                   pairs_per_s=pairs / (med * 1e-3))
        if rs in FLOOR_VALU:
            floor = pairs / 64 * FLOOR_VALU[rs] * 4 / (SIMDS * CLOCK_HZ) * 1e3
            row.update(valu_per_pair=FLOOR_VALU[rs], floor_ms=floor, floor_share=floor / med)
        out["every_range" if every else "listed_ranges"] = row
    print(json.dumps(out), flush=True)


def quality(args):
    import numpy as np
    import torch

    from fwav import engine, synth
    dev = torch.device("cuda", 0)
    signals = {"speech_like(1.5, 44100) tile 2048": (synth.speech_like(1.5, 44100), 2048),
               "speech_like(1.5, 44100) tile 1024": (synth.speech_like(1.5, 44100), 1024),
               "sweep(1.0, 16000) tile 1024": (synth.sweep(1.0, 16000), 1024),
               "noise(1.0, 44100) tile 2048": (synth.noise(1.0, 44100), 2048)}
    for name, (sig, tile) in signals.items():
        row = dict(what="quality", signal=name, fit="clipped")
        for cands in ("embedding", "all"):
            r = engine.compress_device(torch.from_numpy(sig).to(dev), tile, 32, keep_intermediates=True, fit="clipped",
                                       candidates=cands)
            torch.cuda.synchronize()
            rs = r.range_size
            ranges = r.ranges.cpu().numpy().reshape(-1, rs)
            err = r.err.cpu().numpy()
            ok = np.isfinite(err)
            sig2 = (ranges[ok].astype(np.float64) ** 2).sum()
            rec, ran, _ = engine.decompress_device(r.idx, r.s, r.o, r.sym, r.pool, r.n_ranges, rs, s_damping=1e-6)
            noise = ((rec.cpu().numpy().reshape(-1, rs)[ok].astype(np.float64) - ranges[ok]) ** 2).sum()
            row[cands] = dict(fit_snr_db=float(10 * np.log10(sig2 / (err[ok].astype(np.float64) ** 2).sum())),
                              decoded_searched_snr_db_s_damping_1e_06=float(10 * np.log10(sig2 / noise)),
                              iterations=ran, searched=int(ok.sum()))
        row["n_ranges"], row["n_domains"] = r.n_ranges, r.n_domains
        print(json.dumps(row), flush=True)


def run(args):
    """Each GPU step a process of its own under its own time limit; a step that fails ends the chain."""
    os.makedirs(os.path.join(ROOT, args.out), exist_ok=True)
    me = f"{sys.executable} {os.path.join('tools', 'bench_affine_all.py')}"
    steps = [(300, f"{me} time --speech 1.5 --every", "time_speech.log"),
             (300, f"{me} quality", "quality.log"),
             (600, f"{me} time --config cfg2 --every --reps 3", "time_cfg2.log")]
    chain = " && ".join(f"timeout -k 10 {lim} {cmd} > {os.path.join(args.out, log)} 2>&1" for lim, cmd, log in steps)
    return subprocess.call(["bash", "-c", "set -o pipefail; " + chain], cwd=ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("time", "quality", "run"))
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--speech", type=float, default=None, help="a speech_like signal of this many seconds at tile 1024")
    ap.add_argument("--fit", default="clipped", choices=("reference", "clipped"))
    ap.add_argument("--every", action="store_true", help="also time the call with every range listed")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "affine_all"))
    args = ap.parse_args()
    if args.what == "run":
        sys.exit(run(args))
    import __graft_entry__
    __graft_entry__.build()
    {"time": time_shape, "quality": quality}[args.what](args)


if __name__ == "__main__":
    main()
