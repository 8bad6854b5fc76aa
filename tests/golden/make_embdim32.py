"""Generate the emb_dim = 32 fixtures under tests/golden/ from the REFERENCE itself (CPU only, where the reference
is installed; never on a GPU box).

Run:  python tests/golden/make_embdim32.py

The reference is imported and driven stage by stage exactly as make_golden.py does (same inert librosa, same
in-process cpu_worker / _flush_gpu_batch calls), with ``emb_dim=32`` and the module global ``top_k = 32`` (the
reference ignores the ``top_k=`` keyword, quirk Q2).  Each ``embdim32_<case>.npz`` holds only data:

  params      json: framerate, sampwidth, tile, rs, step, thr, K, n_ranges, n_domains, original_len, blas_threads (the
              OpenBLAS thread count of the generating process; every case has 32·n_domains < 460,800, where OpenBLAS
              runs sgemv on one thread whatever that count)
  signal      f32[N]            input (within [−1, 1], so a float32 WAV of it reads back bit for bit)
  emb_sha256  sha256 of build_domain_embeddings(emb_dim=32)'s f32[nd, 32] bytes (the whole table, bit for bit)
  emb_rows    i32[...], emb_sub f32[..., 32]   every 8th row of it and the last (to locate a mismatch)
  cand_sha256 sha256 of cpu_worker's candidates i32[nr, 32] (fractal.py:556-632); cand_rows / cand_sub: every 8th row
  m_idx, m_s, m_o, m_sym, m_err  the match tuples of _process_gpu_batch (fractal.py:757-850), one per range
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ListQueue, _import_reference  # noqa: E402

REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import fractal_oracle as O  # noqa: E402

K = 32
DIM = 32


def noise_tones(n: int, sr: int, seed: int) -> np.ndarray:
    """Gaussian noise plus three tones, with a stretch of digital silence (pruned ranges)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = 0.08 * rng.normal(0.0, 1.0, n)
    for f, a in ((220.0, 0.25), (1370.0, 0.15), (5210.0, 0.1)):
        x += a * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    x[n // 3:n // 3 + 600] = 0.0
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def periodic(n: int, period: int, seed: int) -> np.ndarray:
    """An exactly periodic signal (one random period of harmonics repeated): domains one period apart are identical,
    so their scores tie exactly."""
    rng = np.random.default_rng(seed)
    t = np.arange(period, dtype=np.float64) / period
    one = sum(a * np.sin(2 * np.pi * h * t + rng.uniform(0, 2 * np.pi)) for h, a in ((1, 0.3), (3, 0.2), (7, 0.1)))
    one = one.astype(np.float32)
    return np.tile(one, n // period + 1)[:n].copy()


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def staged(F, signal, tile, thr, framerate, sampwidth):
    rs = max(4, tile // 256)
    step = max(1, rs // 4)
    vm = F.voiced_detection(signal, frame_size=rs * 2, energy_threshold=thr)
    ws = signal * vm
    orig = len(ws)
    pad = (rs - orig % rs) % rs
    if pad:
        ws = np.pad(ws, (0, pad), mode="reflect")
    nr = len(ws) // rs
    ranges = ws.reshape(nr, rs)
    tmp = tempfile.mkdtemp()
    dpath, nd = F.build_domains_memmap(signal, tile, rs, step, block_size=500, tmpdir=tmp)
    epath = F.build_domain_embeddings(dpath, nd, rs, emb_dim=DIM, block_size=4096, tmpdir=tmp)
    emb = np.array(np.memmap(epath, dtype="float32", mode="r", shape=(nd, DIM)))
    pool_mm = np.memmap(dpath, dtype="float32", mode="r", shape=(nd, rs))
    assert DIM * nd < 460800, "keep the fixtures below OpenBLAS's threading threshold"
    F.top_k = K
    q = ListQueue()
    F.cpu_worker(idx_slice=np.arange(nr), ranges=ranges,
                 range_embs=np.memmap(epath, dtype="float32", mode="r", shape=(nr, DIM)),
                 domain_embs_path=epath, n_domains=nd, emb_dim=DIM, candidate_queue=q,
                 ann_index_path=None, energy_thresh=thr, fast_mode=True, batch_size=128)
    pairs = [p for b in q.items if b is not None for p in b]
    assert len(pairs) == nr
    cand = np.stack([c for _, c in sorted(pairs, key=lambda t: t[0])]).astype(np.int32)
    rq = ListQueue()
    for s in range(0, nr, 512):
        F._flush_gpu_batch(pairs[s:s + 512], ranges, pool_mm, rq, use_gpu=False)
    res = dict(rq.items)
    matches = [res[i] for i in range(nr)]
    erows = np.unique(np.r_[np.arange(0, nd, 8), nd - 1]).astype(np.int32)
    crows = np.unique(np.r_[np.arange(0, nr, 8), nr - 1]).astype(np.int32)
    params = dict(framerate=framerate, sampwidth=sampwidth, tile=tile, rs=rs, step=step, thr=thr, K=K, n_ranges=int(nr),
                  n_domains=int(nd), original_len=int(orig), blas_threads=int(O.blas_threads()))
    out = dict(params=np.array(json.dumps(params)), signal=signal, emb_sha256=np.array(sha(emb)), emb_rows=erows,
               emb_sub=emb[erows], cand_sha256=np.array(sha(cand)), cand_rows=crows, cand_sub=cand[crows],
               m_idx=np.array([m[0] for m in matches], np.int32), m_s=np.array([m[1] for m in matches], np.float32),
               m_o=np.array([m[2] for m in matches], np.float32), m_sym=np.array([m[3] for m in matches], np.uint8),
               m_err=np.array([m[4] for m in matches], np.float32))
    for p in (dpath, epath):
        os.remove(p)
    return out, params


def main():
    F = _import_reference()
    cases = {
        # name: (signal, framerate, sampwidth, tile): range sizes 4, 8 and 16, and exact ties at range size 8
        "t1024": (noise_tones(12000, 22050, 11), 22050, 4, 1024),
        "t2048": (noise_tones(14000, 44100, 12), 44100, 4, 2048),
        "t4096": (noise_tones(16000, 44100, 13), 44100, 4, 4096),
        "periodic2048": (periodic(12288, 96, 14), 44100, 4, 2048),
    }
    for name, (sig, fr, sw, tile) in cases.items():
        out, params = staged(F, sig, tile, 1e-4, fr, sw)
        fp = os.path.join(HERE, f"embdim32_{name}.npz")
        np.savez_compressed(fp, **out)
        print(name, params, os.path.getsize(fp), "bytes", flush=True)


if __name__ == "__main__":
    main()
