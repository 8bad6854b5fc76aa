"""Generate tests/golden/front_edges.npz from the REFERENCE itself (the development container only; see make_golden.py
for how the reference is imported — the inert ``librosa`` stub).

Run:  python tests/golden/make_front_edges.py

The inputs come from tests/front_edges.py; every output is what the reference's own function returns for them.  The
file holds only data:
  params                 JSON: the recorded shapes and cases, SHA-256 of every built signal that is not stored itself
  rows_rs<rs>            f32[67, rs]      embed_rows(rs)
  emb_rs<rs>_w<w>        f32[67, w]       multi_head_embedding(row, tonal_k=w/2, transient_k=w/2) per row
                                          (fractal.py:166-208, 154-164)
  vm_f<frame>_n<nf>_t<tail>_w<window>     u8[nf]: voiced_detection's mask, one value per frame (fractal.py:880-909)
  tiny_sig_<n>, tiny_vm_<n>               the signals of 1 … 9 samples (frame 8) and their per-frame masks
  eq_thr_<k> f32[2], eq_vm_<k> u8[nf]     threshold-equality case k of front_edges.EQUAL_CASES: (hi, lo) — each the
                                          smoothed energy of a frame, so that `e > hi` and `e < lo` meet equality — and
                                          the mask for them
  pool_rs<rs>_s<step>_bl<bl>  f32[70, rs] build_domains_memmap's rows for pool_signal(bl, rs, step) (fractal.py:285-334)

The archive is written with fixed time stamps, so that a second run reproduces the committed file byte for byte."""
from __future__ import annotations

import io
import json
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _import_reference  # noqa: E402

import front_edges as FE  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

F32 = np.float32
MAX_NAN_ROWS = 9       # of the 67 reference rows of an embedding shape (a NaN matches any NaN: keep them few)
MIN_FINITE_POOL = 30   # of the 70 rows of a pool fixture


def frame_mask(F, sig, frame, window, hi=FE.VOICED_THR, lo=None):
    vm = F.voiced_detection(sig, frame_size=frame, energy_threshold=hi, smooth_window=window, low_threshold=lo)
    assert len(vm) == len(sig)
    return np.ascontiguousarray(vm[::frame]).astype(np.uint8)


def equality_case(F, sig, frame):
    """→ (hi, lo, mask): hi and lo among the smoothed energies such that the reference's mask changes when hi moves
    one float down (the frame at hi turns voiced) and when lo moves one float up (the frame at lo turns unvoiced)."""
    e = np.unique(O.smooth5(O.frame_energies(sig, frame)))
    e = e[e > 0]
    zero, big = F32(0), F32(np.inf)
    for hi in e[int(0.4 * len(e)):int(0.95 * len(e))][::max(1, len(e) // 60)]:
        for lo in e[int(0.1 * len(e)):][::max(1, len(e) // 60)]:
            if not lo < hi:
                break
            base = frame_mask(F, sig, frame, 5, float(hi), float(lo))
            up = frame_mask(F, sig, frame, 5, float(np.nextafter(hi, zero)), float(lo))
            dn = frame_mask(F, sig, frame, 5, float(hi), float(np.nextafter(lo, big)))
            if not np.array_equal(base, up) and not np.array_equal(base, dn):
                return F32(hi), F32(lo), base
    raise AssertionError("no threshold pair on which equality decides the mask")


def write_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps (numpy's own writer stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    F = _import_reference()
    out, digests = {}, {}

    # ---- embedding
    nan_rows = {}
    for rs, w in FE.EMBED_SHAPES:
        rows, names = FE.embed_rows(rs)
        out[f"rows_rs{rs}"] = rows
        with np.errstate(all="ignore"):
            emb = np.stack([F.multi_head_embedding(r, tonal_k=w // 2, transient_k=w // 2) for r in rows])
        assert emb.dtype == F32 and emb.shape == (FE.N_ROWS, w)
        bad = np.isnan(emb).any(axis=1)
        nan_rows[f"rs{rs}_w{w}"] = [names[i] for i in np.nonzero(bad)[0]]
        assert bad.sum() <= MAX_NAN_ROWS, (rs, w, nan_rows[f"rs{rs}_w{w}"])
        out[f"emb_rs{rs}_w{w}"] = emb
        print(f"embedding rs {rs} width {w}: {int(bad.sum())} rows with a NaN", flush=True)

    # ---- voiced mask
    stats = {}
    for frame, nf, tail, window in FE.voiced_cases(FE.FIXTURE_FRAMES):
        sig = FE.voiced_signal(frame, nf, tail)
        tag = f"f{frame}_n{nf}_t{tail}_w{window}"
        digests["voiced_" + tag] = FE.digest(sig)
        vm = frame_mask(F, sig, frame, window)
        assert len(vm) == nf
        out["vm_" + tag] = vm
        if nf == 1025 and tail == 0 and window == 5:
            e = O.smooth5(O.frame_energies(sig, frame))
            stats[f"frame {frame}"] = [int((e > F32(1e-4)).sum()), int((e < F32(5e-5)).sum()),
                                       int(((e <= F32(1e-4)) & (e >= F32(5e-5))).sum())]
    print("1025 frames [above hi, below lo, keep]:", stats, flush=True)
    for n in FE.TINY_LENGTHS:
        sig = FE.tiny_signal(n)
        out[f"tiny_sig_{n}"] = sig
        out[f"tiny_vm_{n}"] = frame_mask(F, sig, 8, 5)
    for k, (frame, nf, tail) in enumerate(FE.EQUAL_CASES):
        sig = FE.voiced_signal(frame, nf, tail)
        hi, lo, vm = equality_case(F, sig, frame)
        out[f"eq_thr_{k}"] = np.array([hi, lo], F32)
        out[f"eq_vm_{k}"] = vm
        print(f"equality case {k}: frame {frame}, {nf} frames, hi {hi!r}, lo {lo!r}", flush=True)

    # ---- pool
    tmp = tempfile.mkdtemp()
    try:
        for rs, step in FE.POOL_CONFIGS:
            for bl in FE.POOL_BL_FIXTURE:
                sig, tile = FE.pool_signal(bl, rs, step)
                tag = f"rs{rs}_s{step}_bl{bl}"
                digests["pool_" + tag] = FE.digest(sig)
                with np.errstate(all="ignore"):
                    path, nd = F.build_domains_memmap(sig, tile, rs, step, block_size=32, tmpdir=tmp)
                assert nd == FE.N_DOMAINS
                pool = np.array(np.memmap(path, dtype="float32", mode="r", shape=(nd, rs)))
                finite = int(np.isfinite(pool).all(axis=1).sum())
                assert finite >= MIN_FINITE_POOL, (tag, finite)
                out["pool_" + tag] = pool
                print(f"pool {tag}: {finite} of {nd} rows finite", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    out["params"] = np.array(json.dumps(dict(
        n_rows=FE.N_ROWS, embed_shapes=[list(s) for s in FE.EMBED_SHAPES], nan_rows=nan_rows,
        voiced=[list(c) for c in FE.voiced_cases(FE.FIXTURE_FRAMES)], tiny=list(FE.TINY_LENGTHS),
        equal=[list(c) for c in FE.EQUAL_CASES], pool_configs=[list(c) for c in FE.POOL_CONFIGS],
        pool_bl=list(FE.POOL_BL_FIXTURE), inputs=digests), sort_keys=True))
    path = os.path.join(HERE, "front_edges.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
