"""Generate tests/golden/affine_edges.npz from the REFERENCE itself (this container only; see make_golden.py for how
the reference is imported).

Run:  python tests/golden/make_affine_edges.py

For every shape of tests/affine_edges.FIXTURE_SHAPES the edge table of tests/affine_edges.build (all-(−1) rows, −1
tails, constant tiles, mirror pairs, palindromes, clipped s, overflow, inf, NaN, tiny values, then random rows) goes
through the reference's own ``_flush_gpu_batch(use_gpu=False)`` (fractal.py:852-870 → _process_gpu_batch :757-850) at
s_clip 16, 0.5 and −16.  The file holds only data: per shape the inputs (ranges, cand, pool) and the reference's five
outputs per s_clip."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import ListQueue, _import_reference  # noqa: E402

import affine_edges as AE  # noqa: E402

S_CLIPS = (16.0, 0.5, -16.0)


def main():
    F = _import_reference()
    out = {"shapes": np.array(AE.FIXTURE_SHAPES, np.int32), "s_clips": np.array(S_CLIPS, np.float64)}
    for rs, K in AE.FIXTURE_SHAPES:
        ranges, cand, pool, _ = AE.build(rs, K)
        tag = f"rs{rs}_k{K}"
        out[f"ranges_{tag}"], out[f"cand_{tag}"], out[f"pool_{tag}"] = ranges, cand, pool
        for ci, sc in enumerate(S_CLIPS):
            q = ListQueue()
            with np.errstate(all="ignore"):
                F._flush_gpu_batch([(i, cand[i]) for i in range(len(cand))], ranges, pool, q, use_gpu=False, s_clip=sc)
            res = dict(q.items)
            m = [res[i] for i in range(len(cand))]
            for j, (nm, dt) in enumerate((("idx", np.int32), ("s", np.float32), ("o", np.float32), ("sym", np.uint8),
                                          ("err", np.float32))):
                out[f"{nm}_{tag}_c{ci}"] = np.array([t[j] for t in m], dt)
        print(tag, "ok", flush=True)
    np.savez_compressed(os.path.join(HERE, "affine_edges.npz"), **out)


if __name__ == "__main__":
    main()
