"""compress_audio(fit="clipped") restated in numpy (test helper, shared by tests/test_fit_clipped.py and
tests/test_gpu_fit_clipped.py; no torch).

``slots_clipped`` is the contract of fwav_affine_fit(fit=1), slot by slot: the reference's op order up to the
least-squares scale (oracle.affine_slots), then the clip in front of the offset and the error.  ``select`` is its
selection — a NaN error first, else the smallest error, then the smaller clamped domain index, then unmirrored before
mirrored — and ``affine_clipped`` the five outputs.  Every f32 op is rounded separately and the reductions are numpy's
pairwise sums (O.pw_sum, O.pw_mean)."""
import numpy as np

from oracle import fractal_oracle as O

F32 = np.float32


def slots_clipped(ranges, cand, pool, s_clip=16.0):
    """→ (s, o, err, dom), each (B, 2K) over [K candidates | K mirrored]: s already clipped, err +inf where cand < 0,
    dom the clamped domain index."""
    ranges = np.asarray(ranges, F32)
    safe = np.where(cand < 0, 0, cand)
    dom = pool[safe]
    dsym = np.concatenate([dom, dom[:, :, ::-1]], axis=1)
    rm = O.pw_mean(ranges)[:, None]
    rc = ranges - rm
    dm = O.pw_mean(dsym)[:, :, None]
    dc = dsym - dm
    num = O.pw_sum(dc * rc[:, None, :])
    den = O.pw_sum(dc * dc) + F32(1e-12)
    c = abs(F32(s_clip))
    s = np.clip(num / den, -c, c)
    o = rm - s * dm[:, :, 0]
    diff = (s[:, :, None] * dsym + o[:, :, None]) - ranges[:, None, :]
    err = np.sqrt(O.pw_sum(diff * diff))
    bad = np.concatenate([cand < 0] * 2, axis=1)
    return s, o, np.where(bad, F32(np.inf), err), np.concatenate([safe, safe], axis=1)


def select(err, dom):
    """The winning slot of each row: lexicographic minimum of (NaN first else err, dom, mirrored)."""
    K = err.shape[1] // 2
    mirrored = np.broadcast_to(np.arange(2 * K) >= K, err.shape)
    return np.lexsort((mirrored, dom, np.where(np.isnan(err), -np.inf, err)), axis=1)[:, 0]


def affine_clipped(ranges, cand, pool, s_clip=16.0):
    """fwav_affine_fit(fit=1): SoA (idx, s, o, sym, err)."""
    with np.errstate(all="ignore"):
        s, o, err, dom = slots_clipped(ranges, cand, pool, s_clip)
    j = select(err, dom)
    ar = np.arange(len(j))
    K = cand.shape[1]
    return (dom[ar, j].astype(np.int32), s[ar, j].astype(F32), o[ar, j].astype(F32), (j >= K).astype(np.uint8),
            err[ar, j].astype(F32))


def clipped_error_of_reference_slot(ranges, cand, pool, s_clip=16.0):
    """The error of the tuple O.affine stores — its slot, its s clipped, o and err re-done from that s (the clipped
    formula on the reference's slot), which is what the decoder reproduces."""
    with np.errstate(all="ignore"):
        _, _, e_ref = O.affine_slots(ranges, cand, pool)
        j = np.argmin(e_ref, axis=1)
        _, _, err, _ = slots_clipped(ranges, cand, pool, s_clip)
    return err[np.arange(len(j)), j]


def tuple_error(ranges, pool, idx, s, o, sym):
    """‖(s·D + o) − R‖₂ of stored tuples, D = pool[idx] (mirrored where sym), in float64: what a decoder that applies
    the stored s reproduces (+inf where idx < 0 or the result is not a number)."""
    idx = np.asarray(idx)
    tiles = np.asarray(pool, np.float64)[np.where(idx < 0, 0, idx)]
    tiles = np.where(np.asarray(sym).astype(bool)[:, None], tiles[:, ::-1], tiles)
    with np.errstate(all="ignore"):
        d = np.asarray(s, np.float64)[:, None] * tiles + np.asarray(o, np.float64)[:, None] - np.asarray(ranges, np.float64)
        e = np.sqrt((d * d).sum(axis=1))
    return np.where((idx < 0) | np.isnan(e), np.inf, e)


def chunked(fn, ranges, cand, pool, rows=4096, **kw):
    """``fn`` over row chunks (the (B, 2K, rs) intermediates of a whole signal do not fit comfortably at once)."""
    parts = [fn(ranges[a:a + rows], cand[a:a + rows], pool, **kw) for a in range(0, len(ranges), rows)]
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate(p) for p in zip(*parts))
    return np.concatenate(parts)


def snr_db(ranges, err, over):
    """10·log10(Σ‖r‖² / Σ err²) over the rows ``over``."""
    r = np.asarray(ranges, np.float64)[over]
    e = np.asarray(err, np.float64)[over]
    return float(10 * np.log10((r ** 2).sum() / (e ** 2).sum()))


SIGNALS = {"speech": lambda s: s.speech_like(0.5, 44100), "sweep": lambda s: s.sweep(0.5, 16000),
           "noise": lambda s: s.noise(0.4, 44100)}
_RESTATED: dict = {}


def restated(name, tile, query, K=32, **kw):
    """One signal compressed in numpy, once per argument tuple: the oracle's stages (O.compress for the default query,
    restate_compress of tests/test_gpu_query_range.py for query="range") up to the candidate rows, then both fits.
    → dict(sig, ranges, cand, pool, nr, rs, step, m: the reference fit's tuples (idx, s, o, sym, err), mc: the clipped
    fit's, e_stored / e_stored_c: tuple_error of either — the reference fit stores the clipped s beside the o of the
    unclipped one, so its e_stored is not its err)."""
    key = (name, tile, query, K, tuple(sorted(kw.items())))
    if key not in _RESTATED:
        from fwav import synth
        sig = SIGNALS[name](synth)
        if query == "range":
            from test_gpu_query_range import restate_compress
            c = restate_compress(sig, tile, K, **kw)
            m = c["m"]
        else:
            c = O.compress(sig, tile, K, **kw)
            m = tuple(c[f] for f in ("idx", "s", "o", "sym", "err"))
        ranges, cand, pool = c["ranges"], c["cand"], c["pool"]
        _RESTATED[key] = dict(sig=sig, ranges=ranges, cand=cand, pool=pool, nr=len(ranges), rs=c["rs"], step=c["step"],
                              m=m, mc=chunked(affine_clipped, ranges, cand, pool),
                              e_stored=tuple_error(ranges, pool, *m[:4]))
        _RESTATED[key]["e_stored_c"] = tuple_error(ranges, pool, *_RESTATED[key]["mc"][:4])
    return _RESTATED[key]


def twin_rows(rs, K, seed=0):
    """Rows for tests/affine_edges.build's pool layout: two different indices hold bit-identical tiles, in both slot
    orders, alone and among others, and a twin pair of palindromes (four slots with one error).  → (ranges, cand,
    pool patch {index: source index})."""
    import affine_edges as AE
    rng = np.random.default_rng(77 * rs + K + seed)
    lo, hi = 7, 150                      # pool[hi] := pool[lo]
    plo, phi = AE.P_PAL, 151             # pool[phi] := pool[P_PAL]
    ranges, cand = [], []

    def row(cs, at=0):
        c = np.full(K, -1, np.int32)
        cs = list(cs)[:max(0, K - at)]
        c[at:at + len(cs)] = cs
        ranges.append(rng.normal(0, 0.3, rs).astype(F32))
        cand.append(c)

    row([lo, hi])
    row([hi, lo])
    row([hi, lo], at=max(K - 2, 0))
    row([hi, 33, lo])
    row([phi, plo])
    row([plo, phi])
    row(np.r_[hi, rng.integers(0, AE.N_PLAIN, max(K - 2, 0)), lo])
    return np.stack(ranges), np.stack(cand), {hi: lo, phi: plo}
