"""compress_audio(candidates="all") restated in numpy (test helper, shared by tests/test_candidates_all_cpu.py and
tests/test_gpu_candidates_all.py; no torch).

No new arithmetic: the exhaustive solve is the affine solve of the candidate row 0, 1, …, n_domains − 1, so
``affine_all`` hands that row to the restatements that exist — fit_clipped.affine_clipped (fit 1) and the oracle's
affine (fit 0) — chunked over rows, because a chunk's intermediates are (rows, 2·n_domains, rs)."""
import numpy as np

import fit_clipped as FC
from oracle import fractal_oracle as O

F32 = np.float32
NAMES = ("idx", "s", "o", "sym", "err")
FIT_NAMES = ("reference", "clipped")


def affine_all(ranges, pool, fit, s_clip=16.0, rows=None):
    """fwav_affine_all over every row of ``ranges``: SoA (idx, s, o, sym, err).  ``rows``: the chunk (default: about
    2^22 slot elements per intermediate)."""
    ranges = np.ascontiguousarray(ranges, F32)
    pool = np.ascontiguousarray(pool, F32)
    nd, rs = pool.shape
    if rows is None:
        rows = max(1, (1 << 22) // (2 * nd * rs))
    fn = FC.affine_clipped if fit == 1 else O.affine
    cand1 = np.arange(nd, dtype=np.int32)[None, :]
    with np.errstate(all="ignore"):
        parts = [fn(ranges[a:a + rows], np.repeat(cand1, len(ranges[a:a + rows]), axis=0), pool, s_clip=s_clip)
                 for a in range(0, len(ranges), rows)]
    if not parts:
        return tuple(np.zeros(0, dt) for dt in (np.int32, F32, F32, np.uint8, F32))
    return tuple(np.concatenate(p) for p in zip(*parts))


def pruned_tuple(ranges, pool, fit, s_clip=16.0):
    """What today's path gives a pruned row: the same solve on an all-−1 candidate row."""
    fn = FC.affine_clipped if fit == 1 else O.affine
    with np.errstate(all="ignore"):
        return fn(np.asarray(ranges, F32), np.full((len(ranges), 1), -1, np.int32), pool, s_clip=s_clip)


_RESTATED: dict = {}


def restate_compress_all(sig, tile, fit, energy_thresh=1e-4, fast_mode=True):
    """The oracle's ranges and pool, its prune predicate, affine_all on the kept rows and pruned_tuple on the others.
    → dict(ranges, pool, pruned, rs, step, m: (idx, s, o, sym, err)); once per argument tuple."""
    sig = np.asarray(sig, F32)
    key = (sig.tobytes(), tile, fit, energy_thresh, fast_mode)
    if key not in _RESTATED:
        rs, step = O.geometry(tile)
        vm = O.voiced_detection(sig, frame_size=2 * rs, energy_threshold=energy_thresh)
        ranges, _ = O.form_ranges(sig, vm, rs)
        pool = O.domain_pool(sig, tile, rs, step)
        pruned = O.range_energy_pruned(ranges, energy_thresh, fast_mode)
        pruned = np.broadcast_to(np.asarray(pruned, bool), (len(ranges),))
        kept = affine_all(ranges[~pruned], pool, fit)
        gone = pruned_tuple(ranges[pruned], pool, fit)
        m = []
        for k, g in zip(kept, gone):
            a = np.empty(len(ranges), k.dtype)
            a[~pruned] = k
            a[pruned] = g
            m.append(a)
        _RESTATED[key] = dict(ranges=ranges, pool=pool, pruned=pruned, rs=rs, step=step, m=tuple(m))
    return _RESTATED[key]
