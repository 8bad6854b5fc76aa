"""The one table from (embedding, embedding width, query table) to the C ABI's entry points, and the reference's scalars.

``include/fwav.h`` has three families of search entry points — the plain ones (``emb_dim=16``, range i's query is
domain-embedding row i), the ``*_dim`` ones (``emb_dim=32``) and the ``*_q`` ones (``query="range"``: a query table of
its own) — and two embedding modes ("matrix" / "pocketfft").  Every host (fwav.engine on torch tensors, fwav.hipctypes
on HIP buffers, fwav.ties, fwav.dist) picks among them here and nowhere else.  Torch-free: a device argument is a raw
pointer (``int`` or ``None``), a stream an ``int`` or ``None`` (``tensor.data_ptr()`` or ``DeviceBuffer.value``);
nothing here allocates device memory or synchronises.  Each stage takes the header's arguments in the header's order.
"""
from __future__ import annotations

import numpy as np

from . import geometry  # noqa: F401  range_size, domain_step (fractal.py:1070-1071)
from ._lib import call, size_call

F32 = np.float32

# ------------------------------------------------------------------------------------------ options and their checks
#: embedding → (tables size call, tables call, pool + embedding call).  "matrix": bit-exact at range sizes 4, 8 and
#: 16, an f64 matrix DCT elsewhere; "pocketfft": scipy's own DCT sequence, bit-exact at every supported range size
EMBEDDINGS = {"matrix": ("fwav_embed_tables_size", "fwav_embed_tables", "fwav_pool_embed"),
              "pocketfft": ("fwav_embed_tables_exact_size", "fwav_embed_tables_exact", "fwav_pool_embed_exact")}
#: embedding → the call that embeds rows other than the pool's with the same kernel
EMBED_ROWS = {"matrix": "fwav_embed_rows", "pocketfft": "fwav_embed_rows_exact"}
#: the embedding widths the engine implements (compress_audio's emb_dim): 16, the reference's default, through the
#: plain entry points; 32 through the *_dim entry points of include/fwav.h
EMB_DIMS = (16, 32)
#: query → where range i's query vector comes from: domain-embedding row i (the reference's pipeline, quirk Q1) or
#: the embedding of the range itself (what fractal.py:337-351 computes and the pipeline never calls)
QUERIES = ("domain_row", "range")
#: the largest K of the search with a query table of its own (fwav_sim_topk_q)
QUERY_RANGE_MAX_K = 64
#: tie_order → fwav_tie_check's exact_sets argument ("index" never calls it)
TIE_MODES = {"numpy": 0, "numpy_sets": 1, "numpy_rows": 2, "index": -1}
TIE_REC = 9  # int32 per tie record (kTieRec, fwav_common.h)
#: fit → fwav_affine_fit's fit argument: "reference" selects the slot by the error of the unclipped least-squares
#: scale and clips the stored one afterwards (fractal.py:804-824); "clipped" clips first, so that the error it selects
#: by and stores is the stored tuple's, and breaks ties by (domain, orientation) instead of the slot
FITS = ("reference", "clipped")
#: candidates → the domains the affine solve picks among: the K that the embedding search proposes (the reference's
#: pipeline), or every domain of the pool (fwav_affine_all: the best match the pool holds; no embedding, no search)
CANDIDATES = ("embedding", "all")


def check_embedding(embedding: str, rs: int) -> str:
    """``embedding`` validated for range size ``rs``: ValueError for an unknown mode, and for "pocketfft" at a range
    size with no exact plan (there is no silent fall-back to the matrix DCT)."""
    if embedding not in EMBEDDINGS:
        raise ValueError(f"embedding must be 'matrix' or 'pocketfft', not {embedding!r}")
    if embedding == "pocketfft" and not size_call("fwav_embed_exact_supported", int(rs)):
        raise ValueError(f"embedding='pocketfft' has no exact plan for range size {rs} (supported: 4 to 49 and 50, 54, "
                         "56, 60, 63, 64); use embedding='matrix'")
    return embedding


def check_emb_dim(emb_dim, embedding: str = "matrix") -> int:
    """``emb_dim`` validated: NotImplementedError for a width other than 16 and 32, ValueError for 32 together with
    embedding="pocketfft" (the exact plans are built for heads of 8 coefficients)."""
    if emb_dim not in EMB_DIMS:
        raise NotImplementedError(f"emb_dim={emb_dim!r}: the MI355X engine supports emb_dim 16 and 32")
    if emb_dim != 16 and embedding == "pocketfft":
        raise ValueError("embedding='pocketfft' with emb_dim=32 is out of scope: use embedding='matrix'")
    return int(emb_dim)


def check_query(query: str, emb_dim: int = 16, top_k: int | None = None) -> str:
    """``query`` validated (no device work): ValueError for a name other than "domain_row" and "range", and for "range"
    together with emb_dim=32 or top_k > 64 (neither is built)."""
    if query not in QUERIES:
        raise ValueError(f"query must be 'domain_row' or 'range', not {query!r}")
    if query == "range":
        if emb_dim != 16:
            raise ValueError("query='range' with emb_dim=32 is out of scope: use emb_dim=16")
        if top_k is not None and int(top_k) > QUERY_RANGE_MAX_K:
            raise ValueError(f"query='range' supports top_k <= {QUERY_RANGE_MAX_K}, not {int(top_k)}")
    return query


def check_tie_order(tie_order: str) -> str:
    """``tie_order`` validated: ValueError for a name that TIE_MODES does not hold."""
    if tie_order not in TIE_MODES:
        raise ValueError("tie_order must be 'numpy' (the reference's order of exactly tied scores wherever it decides a"
                         " match), 'numpy_sets' (and wherever it decides a candidate set), 'numpy_rows' (and wherever it"
                         " decides a candidate row's order) or 'index'")
    return tie_order


def check_fit(fit: str) -> str:
    """``fit`` validated (no device work): ValueError for a name other than "reference" and "clipped"."""
    if fit not in FITS:
        raise ValueError(f"fit must be 'reference' or 'clipped', not {fit!r}")
    return fit


def check_candidates(candidates: str) -> str:
    """``candidates`` validated (no device work): ValueError for a name other than "embedding" and "all"."""
    if candidates not in CANDIDATES:
        raise ValueError(f"candidates must be 'embedding' or 'all', not {candidates!r}")
    return candidates


def tie_mode(tie_order: str, fit: str = "reference") -> int:
    """fwav_tie_check's exact_sets for ``tie_order`` under ``fit``.  The check tests the reference's error, so with
    fit="clipped" it cannot tell which K-th place ties leave the match alone: "numpy" then ranks every one of them on
    the host ("numpy_sets"), which makes the candidate sets the reference's; the order inside a set cannot change a
    clipped match."""
    check_tie_order(tie_order)
    if check_fit(fit) == "clipped" and tie_order == "numpy":
        return TIE_MODES["numpy_sets"]
    return TIE_MODES[tie_order]


# ------------------------------------------------------------------------------------------ the reference's scalars
#: np.ones(5) / 5, the smoothing window of voiced_detection (fractal.py:895)
SMOOTH_WINDOW = 5


def voiced_hi(energy_thresh: float) -> float:
    """The threshold a frame's smoothed energy rises above to turn voiced (fractal.py:898), as the float32 it is."""
    return float(F32(energy_thresh))


def voiced_lo(energy_thresh: float) -> float:
    """... and the one it falls below to turn unvoiced again (0.5·thr, :899)."""
    return float(F32(energy_thresh * 0.5))


def prune_thr(energy_thresh: float) -> float:
    """cpu_worker's energy prune (fractal.py:601-603): a range is searched when its mean(r²) reaches 0.75·thr."""
    return float(F32(energy_thresh * 0.75))


def is_silent(sum32) -> bool:
    """np.sum((signal·mask)²) < 1e-8 (fractal.py:1083) on fwav_weighted_energy's sum, numpy's float32 sum bit for bit:
    float32 against float32(1e-8) (NEP 50)."""
    return bool(F32(sum32) < F32(1e-8))


def clip32(s_clip: float) -> float:
    """|s_clip| as the float32 the affine solve and the decoder clip with."""
    return float(abs(F32(s_clip)))


def n_domains_for(n: int, tile_size: int, step: int) -> int:
    return 0 if n < tile_size else (n - tile_size) // step + 1


# ------------------------------------------------------------------------------------------ sizes and host tables
def embed_tables_host(rs: int, embedding: str = "matrix", emb_dim: int = 16) -> np.ndarray:
    """The embedding kernels' host table f64[…] for range size ``rs`` (validated first: check_embedding,
    check_emb_dim)."""
    check_embedding(embedding, rs)
    dim = check_emb_dim(emb_dim, embedding)
    if dim != 16:
        tab = np.zeros(size_call("fwav_embed_tables_dim_size", rs, dim), np.float64)
        call("fwav_embed_tables_dim", rs, dim, tab.ctypes.data)
    else:
        size_fn, fill_fn = EMBEDDINGS[embedding][:2]
        tab = np.zeros(size_call(size_fn, rs), np.float64)
        call(fill_fn, rs, tab.ctypes.data)
    return tab


def emb16_elems(nd: int, emb_dim: int = 16) -> int:
    """Halfs of the search's fp16 table beside ``nd`` embedding rows of ``emb_dim`` columns."""
    return size_call("fwav_emb16_elems", nd) if emb_dim == 16 else size_call("fwav_embh_elems", nd, emb_dim)


def topk_workspace_size(mq: int, nd: int, k: int, *, emb_dim: int = 16, f16: bool = True) -> int:
    """Bytes of the search's workspace for mq queries; the 16-wide exact search (no fp16 table) needs none up to
    K = 64."""
    if emb_dim != 16:
        return size_call("fwav_sim_topk_dim_workspace_size", mq, nd, emb_dim, k)
    return size_call("fwav_sim_topk_workspace_size", mq, nd, k) if (f16 or k > 64) else 0


def compact_rows_cap(nd: int, nr: int) -> int:
    """The most rows fwav_compact_domains can keep: one per range, row 0 when every index is negative."""
    return min(nd, max(nr, 1))


def compact_count(counts) -> int:
    """fwav_compact_domains' ``counts`` (kept rows, entries >= n_domains) → the kept rows; IndexError for an entry out
    of range, as decompress_audio raises it (fractal.py:1414)."""
    m, over = (int(v) for v in counts)
    if over:
        raise IndexError("domain index out of range")
    return m


# ------------------------------------------------------------------------------------------ stage calls
def pool_embed(sig, n, tile, rs, step, tab, pool, emb, emb16, ws, ws_bytes, stream, *, embedding="matrix", emb_dim=16):
    """build_domains_memmap + build_domain_embeddings (fractal.py:285-334, 238-280)."""
    if emb_dim != 16:
        call("fwav_pool_embed_dim", sig, n, tile, rs, step, emb_dim, tab, pool, emb, emb16, ws, ws_bytes, stream)
    else:
        call(EMBEDDINGS[embedding][2], sig, n, tile, rs, step, tab, pool, emb, emb16, ws, ws_bytes, stream)


def embed_rows(rows, n, rs, tab, emb, emb16, stream, *, embedding="matrix"):
    """multi_head_embedding of n rows of rs samples by the pool rows' kernel (query="range": the ranges themselves)."""
    call(EMBED_ROWS[embedding], rows, n, rs, tab, emb, emb16, stream)


def prune(ranges, n, q_offset, rs, thr, fast_mode, emb, nd, k, zero_cand, cand, active, n_active, stream, *,
          emb_dim=16, qemb=None, n_query_rows=0):
    """The energy prune and the all-zero queries of ranges [q_offset, q_offset + n); the query rows are ``emb``'s, or
    with ``qemb`` that table's (``emb`` is then not read)."""
    if qemb is not None:
        call("fwav_prune_q", ranges, n, q_offset, rs, thr, fast_mode, qemb, n_query_rows, nd, k, zero_cand, cand,
             active, n_active, stream)
    elif emb_dim != 16:
        call("fwav_prune_dim", ranges, n, q_offset, rs, thr, fast_mode, emb, nd, emb_dim, k, zero_cand, cand, active,
             n_active, stream)
    else:
        call("fwav_prune", ranges, n, q_offset, rs, thr, fast_mode, emb, nd, k, zero_cand, cand, active, n_active,
             stream)


def sim_topk(emb, emb16, nd, active, n_active, max_q, q_offset, k, threads, cand, ties, ws, ws_bytes, stream, *,
             emb_dim=16, query=None):
    """The top-K search; ``query`` = (qemb, qemb16, n_query_rows, seed_stride) searches with a query table."""
    if query is not None:
        call("fwav_sim_topk_q", emb, emb16, nd, *query, active, n_active, max_q, q_offset, k, threads, cand, ties, ws,
             ws_bytes, stream)
    elif emb_dim != 16:
        call("fwav_sim_topk_dim", emb, emb16, nd, emb_dim, active, n_active, max_q, q_offset, k, threads, cand, ties,
             ws, ws_bytes, stream)
    else:
        call("fwav_sim_topk", emb, emb16, nd, active, n_active, max_q, q_offset, k, threads, cand, ties, ws, ws_bytes,
             stream)


def tie_check(ranges, n_ranges, rs, cand, k, pool, nd, emb, q_offset, threads, ties, max_ties, exact_sets, resolve,
              stream, *, emb_dim=16, qemb=None):
    """Of the rows with exactly tied scores, those that numpy's tie order can change (``exact_sets``: TIE_MODES)."""
    if qemb is not None:
        call("fwav_tie_check_q", ranges, n_ranges, rs, cand, k, pool, nd, emb, qemb, q_offset, threads, ties, max_ties,
             exact_sets, resolve, stream)
    elif emb_dim != 16:
        call("fwav_tie_check_dim", ranges, n_ranges, rs, cand, k, pool, nd, emb, emb_dim, q_offset, threads, ties,
             max_ties, exact_sets, resolve, stream)
    else:
        call("fwav_tie_check", ranges, n_ranges, rs, cand, k, pool, nd, emb, q_offset, threads, ties, max_ties,
             exact_sets, resolve, stream)


def score_rows(emb, nd, rows, n_rows, q_offset, threads, scores, stream, *, emb_dim=16, qemb=None):
    """Exact score rows f32[n_rows·nd] of the listed (local) rows, in the reference's own sgemv order."""
    if qemb is not None:
        call("fwav_score_rows_q", emb, nd, qemb, rows, n_rows, q_offset, threads, scores, stream)
    elif emb_dim != 16:
        call("fwav_score_rows_dim", emb, nd, emb_dim, rows, n_rows, q_offset, threads, scores, stream)
    else:
        call("fwav_score_rows", emb, nd, rows, n_rows, q_offset, threads, scores, stream)


def affine(ranges, n, rs, cand, k, pool, nd, s_clip, outs5, stream, *, fit="reference"):
    """_process_gpu_batch (fractal.py:757-850) into ``outs5`` = (idx, s, o, sym, err); ``fit``: FITS."""
    if fit == "reference":
        call("fwav_affine", ranges, n, rs, cand, k, pool, nd, s_clip, *outs5, stream)
    else:
        call("fwav_affine_fit", ranges, n, rs, cand, k, pool, nd, s_clip, *outs5, FITS.index(check_fit(fit)), stream)


def prune_energy(ranges, n, rs, thr, fast_mode, active, n_active, stream):
    """The energy prune alone (fwav_prune's first rule, by its code): the kept local ranges into ``active``."""
    call("fwav_prune_energy", ranges, n, rs, thr, fast_mode, active, n_active, stream)


def affine_all_workspace_size(mq: int, nd: int, rs: int) -> int:
    """Bytes of fwav_affine_all's workspace for a list of at most mq ranges (0 when the domain axis is not split)."""
    return size_call("fwav_affine_all_workspace_size", mq, nd, rs)


def affine_all(ranges, n, rs, active, n_active, max_q, pool, nd, s_clip, outs5, ws, ws_bytes, stream, *,
               fit="reference"):
    """The affine solve of the listed ranges over every domain of the pool into ``outs5`` = (idx, s, o, sym, err):
    fwav_affine_fit's result for the candidate row 0 … nd − 1; ``active`` None lists every range."""
    call("fwav_affine_all", ranges, n, rs, active, n_active, max_q, pool, nd, s_clip, *outs5,
         FITS.index(check_fit(fit)), ws, ws_bytes, stream)


def tie_fixup(rows, n, new_cand, k, cand, ranges, rs, rsub, tmp5, outs5, pool, nd, s_clip, stream, *, fit="reference"):
    """numpy's candidate rows written back and their matches re-solved, three launches: ``new_cand`` scattered into
    ``cand`` and the rows' ranges gathered into ``rsub``, the affine solve of those n rows (in the call's own ``fit``)
    into ``tmp5``, its outputs scattered into ``outs5`` = (idx, s, o, sym, err)."""
    call("fwav_tie_rows_in", rows, n, new_cand, k, cand, ranges, rs, rsub, stream)
    affine(rsub, n, rs, new_cand, k, pool, nd, s_clip, tmp5, stream, fit=fit)
    call("fwav_tie_rows_out", rows, n, *tmp5, *outs5, stream)


def decode_exact(prev, nxt, n, eps, t, deltas, state, stream):
    """The reference's Δ of iteration t between two reconstructions, in its own sdot order (fractal.py:1460-1465)."""
    call("fwav_decode_exact", prev, nxt, n, eps, t, deltas, state, stream)


def decode(idx, s, o, sym, nr, rs, pool, nd, iterations, eps, s_clip, s_damping, a, b, deltas, state, ws, ws_bytes,
           stream, *, read_state, snapshot):
    """decompress_audio's loop (fractal.py:1378-1473) between the buffers ``a`` and ``b``: fwav_decode_from; where the
    f64 Δ cannot decide the reference's Δ < eps it stops (state 2) for decode_exact, and when the reference goes on
    (state 3) the loop resumes from a copy of the result.  ``read_state()`` returns ``state``'s 4 ints once the stream
    has run (the host synchronises its own way); ``snapshot(result_ptr)`` returns the pointer of a copy the host keeps.
    ``deltas`` is f64[iterations].  Returns (the result is in b, iterations run)."""
    done, init = 0, None
    while True:
        call("fwav_decode_from", idx, s, o, sym, nr, rs, pool, nd, iterations - done, eps, s_clip, s_damping, init, a, b,
             deltas + 8 * done, state, ws, ws_bytes, stream)
        code, ran, in_b, _ = (int(v) for v in read_state())
        out, other = (b, a) if in_b == 1 else (a, b)
        if code == 2:
            decode_exact(other, out, nr * rs, eps, ran - 1, deltas + 8 * done, state, stream)
            if int(read_state()[0]) == 3 and done + ran < iterations:
                init = snapshot(out)
                done += ran
                continue
        return in_b == 1, done + ran
