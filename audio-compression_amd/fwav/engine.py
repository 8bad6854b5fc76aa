"""Device pipeline: the hot path of ``compress_audio`` / ``decompress_audio`` on one MI355X.

Everything between the input signal and the match arrays stays in HBM and runs on one HIP stream through
the C-ABI of ``libfwav.so`` (``include/fwav.h``); torch only provides device memory and the stream.  There
is no CPU fallback: without the library or a device every call raises :class:`~fwav._lib.FwavError`.  This host
allocates, picks the streams and decides where to synchronise; which entry point serves an embedding mode, a width
or a query table, and the reference's scalars, are fwav.stages'.

Reference map (``/root/reference/fractal.py``):
  voiced_detection :880-909 + range formation :1074-1112  → fwav_voiced_ranges
  silent-input test :1083                                  → fwav_weighted_energy (f64 partials)
  build_domains_memmap :285-334 + build_domain_embeddings :238-280 → fwav_pool_embed
  cpu_worker energy prune :601-603, pad :622               → fwav_prune
  linear top-K :535-541, 617-620                           → fwav_sim_topk (+ fwav_tie_check / fwav.ties for exact ties)
  the same stages on rows of emb_dim = 32 columns (:275)   → fwav_pool_embed_dim, fwav_prune_dim, fwav_sim_topk_dim, …
  _process_gpu_batch :757-850                              → fwav_affine
  (no counterpart; opt-in) the same solve selecting by the stored tuple's error → fwav_affine_fit (fit="clipped")
  (no counterpart; opt-in) the same solve over every domain of the pool → fwav_prune_energy + fwav_affine_all
                                                             (candidates="all")
  decompress_audio :1378-1473                              → fwav_decode
  (no counterpart; opt-in) the pool rows that :1414 reads   → fwav_compact_domains (compact_device / compact_arrays)
  (no counterpart call; opt-in) range_candidates_from_embedding :337-351, each range's own embedding as its query
                                                           → fwav_embed_rows + fwav_prune_q / fwav_sim_topk_q / …
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import _lib, geometry, stages, ties as _ties  # noqa: F401  geometry: re-exported
from .nporder import zero_query_candidates  # noqa: F401  (Q11 rows; re-exported)
from ._lib import FwavError, call, size_call
from .stages import (CANDIDATES, EMB_DIMS, EMBEDDINGS, FITS, QUERIES, QUERY_RANGE_MAX_K, TIE_MODES, TIE_REC,  # noqa: F401  re-exported
                     check_candidates, check_emb_dim, check_embedding, check_fit, check_query, n_domains_for)


def require_device(device=None) -> torch.device:
    _lib.lib()
    if not torch.cuda.is_available():
        raise FwavError("no HIP device visible: the fwav engine has no CPU path")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_TABLES: dict = {}


def embed_tables(rs: int, device: torch.device, embedding: str = "matrix", emb_dim: int = 16) -> torch.Tensor:
    """stages.embed_tables_host on ``device`` (one copy per range size, width, device and mode)."""
    key = (rs, emb_dim, str(device), embedding)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(stages.embed_tables_host(rs, embedding, emb_dim)).to(device)
    return _TABLES[key]


_ZERO_CAND_DEV: dict = {}


def _zero_cand_device(n_domains: int, top_k: int, device: torch.device) -> torch.Tensor:
    key = (int(n_domains), int(top_k), str(device))
    if key not in _ZERO_CAND_DEV:
        _ZERO_CAND_DEV[key] = torch.from_numpy(zero_query_candidates(n_domains, top_k)).to(device)
    return _ZERO_CAND_DEV[key]


@dataclasses.dataclass
class DeviceCompressed:
    """Result of :func:`compress_device`.  Device tensors (final once ``wait()`` returns)."""

    n_ranges: int
    range_size: int
    tile_size: int
    domain_step: int
    energy_thresh: float
    original_len: int
    n_domains: int
    top_k: int
    shard: tuple[int, int]
    ranges: Optional[torch.Tensor] = None
    pool: Optional[torch.Tensor] = None
    emb: Optional[torch.Tensor] = None
    qemb: Optional[torch.Tensor] = None  # query="range": the ranges' own embeddings f32[n_ranges·16] (keep_intermediates)
    cand: Optional[torch.Tensor] = None
    idx: Optional[torch.Tensor] = None
    s: Optional[torch.Tensor] = None
    o: Optional[torch.Tensor] = None
    sym: Optional[torch.Tensor] = None
    err: Optional[torch.Tensor] = None
    n_active: Optional[torch.Tensor] = None
    energy_partial: Optional[torch.Tensor] = None
    ties: Optional[torch.Tensor] = None  # fwav_sim_topk's tie list (keep_intermediates)
    resolved: Optional[torch.Tensor] = None  # local rows re-ranked with numpy's order (keep_intermediates)
    search_ws: Optional[torch.Tensor] = None  # fwav_sim_topk's workspace after the call (keep_intermediates, one launch)
    n_ties: int = 0          # queries whose top K + 1 scores hold exact ties
    n_resolved: int = 0      # of those, rows re-ranked with numpy's own tie order (fwav.ties)
    empty: bool = False
    pending: Optional[object] = None  # deferred tie resolution (compress_device(defer_ties=True)): a Future
    apply: Optional[object] = None    # ... and its last step, run by wait() on the call's own stream
    stream: Optional[object] = None   # the torch stream the call's kernels were queued on
    kept: Optional[torch.Tensor] = None  # compact_device: the original index of each pool row, int32[n_domains]

    def wait(self) -> "DeviceCompressed":
        """Complete a deferred tie resolution (no-op otherwise); the outputs are final afterwards.  The fix-up runs on
        the call's own stream, after its search and affine solve, and whichever stream is current here waits for it
        (so both the call's stream and the caller's see final outputs)."""
        if self.pending is not None:
            staged = self.pending.result()
            self.pending = None
            if staged is not None and self.apply is not None:
                st = self.stream if self.stream is not None else torch.cuda.current_stream()
                caller = torch.cuda.current_stream(st.device)
                with torch.cuda.device(st.device), torch.cuda.stream(st):
                    self.apply(*staged)
                if caller != st:
                    ev = torch.cuda.Event()
                    ev.record(st)
                    caller.wait_event(ev)
            self.apply = None
        return self

    def is_silent(self) -> bool:
        """np.sum((signal·mask)²) < 1e-8 (fractal.py:1083): the device computes numpy's float32 sum bit-exactly
        (stages.is_silent)."""
        return self.energy_partial is None or stages.is_silent(self.energy_partial.cpu().numpy()[0])


def _mark(ev, name: str, end: bool = False):
    """Record a HIP event on the current stream into ev[name] = [start, end] (bench instrumentation)."""
    if ev is None:
        return
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    ev.setdefault(name, []).append(e)


def _empty(n, rs, tile, step, thr, k) -> DeviceCompressed:
    return DeviceCompressed(0, rs, tile, step, thr, n, 0, k, (0, 0), empty=True)


def _voiced_ranges(sig, n, rs, energy_thresh, st) -> torch.Tensor:
    """fwav_voiced_ranges on the stream ``st``: the voiced-masked, reflect-padded ranges f32[nr·rs]."""
    nr, frame = -(-n // rs), 2 * rs
    ws_n = size_call("fwav_voiced_workspace_size", n, frame)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=sig.device)
    ranges = torch.empty(nr * rs, dtype=torch.float32, device=sig.device)
    call("fwav_voiced_ranges", sig.data_ptr(), n, rs, frame, stages.SMOOTH_WINDOW, stages.voiced_hi(energy_thresh),
         stages.voiced_lo(energy_thresh), ranges.data_ptr(), nr, None, ws.data_ptr(), ws_n, st)
    return ranges


def ranges_device(sig: torch.Tensor, tile_size: int, energy_thresh: float = 1e-4) -> tuple[torch.Tensor, int, int]:
    """The ranges alone (voiced detection + range formation, fractal.py:880-909, 1074-1112) on the current stream of
    ``sig``'s device: (ranges f32[nr·rs], nr, rs) — what fwav.dist needs to balance the shards before a compress."""
    if sig.dim() != 1 or sig.dtype != torch.float32 or not sig.is_cuda:
        raise ValueError("ranges_device expects a 1-D float32 device tensor")
    with torch.cuda.device(sig.device):
        sig = sig.contiguous()
        n = sig.numel()
        rs, _ = geometry(tile_size)
        if n == 0:
            raise ValueError("a cannot be empty")
        r = _voiced_ranges(sig, n, rs, energy_thresh, _stream(sig.device))
        return r, -(-n // rs), rs


def compress_device(sig: torch.Tensor, *args, **kwargs) -> DeviceCompressed:
    """Run the compress hot path on ``sig``'s device (made current for the call: the C ABI's per-device plans and
    kernel attributes are taken from the current HIP device).  See :func:`_compress_device`."""
    with torch.cuda.device(sig.device):
        return _compress_device(sig, *args, **kwargs)


def _compress_device(sig: torch.Tensor, tile_size: int, top_k: int, energy_thresh: float = 1e-4,
                     fast_mode: bool = True, s_clip: float = 16.0, shard: Optional[tuple[int, int]] = None,
                     keep_intermediates: bool = False, events: Optional[dict] = None,
                     search: str = "f16", on_pool=None, blas_threads: Optional[int] = None,
                     tie_order: str = "numpy", defer_ties: bool = False,
                     sub_blocks: Optional[int] = None, embedding: str = "matrix",
                     emb_dim: int = 16, query: str = "domain_row", fit: str = "reference",
                     candidates: str = "embedding") -> DeviceCompressed:
    """Run the compress hot path on ``sig`` (1-D float32 tensor on a HIP device).

    ``shard=(lo, hi)`` restricts candidate search and the affine solve to ranges ``[lo, hi)`` (the
    multi-GPU path; a callable ``shard(ranges, n_ranges, range_size) -> (lo, hi)`` picks them once the voiced-masked
    ranges exist); voiced detection, pool and embeddings are always computed for the whole signal,
    because query vectors are domain-embedding rows (quirk Q1) and the voiced state is a scan over the
    whole signal.  Raises ValueError for the reference's own error cases (empty input; n_ranges >
    n_domains).  ``on_pool(pool)``, when given, is called right after the pool kernel is queued (the API
    starts the pool's device→host copy there, on a side stream, so that it overlaps the search).
    ``blas_threads``: the OpenBLAS thread count whose sgemv order the scores follow (default: this process's,
    fwav.ties.blas_threads).  ``tie_order="numpy"`` re-ranks the rows whose match depends on the order of exactly
    equal scores with numpy's own calls, as the reference does (one host synchronisation to read the count), so every
    match tuple is the reference's; ``"numpy_sets"`` also re-ranks every row with a tie at the K-th place, so that
    the candidate sets are the reference's too; ``"numpy_rows"`` re-ranks every row with any exact tie in its top K + 1,
    so that every candidate row, order included, is the reference's (a parity mode: thousands of host rows at cfg2);
    ``"index"`` keeps the device's (score desc, index asc) order (no
    synchronisation).  ``defer_ties=True`` hands that host step to a background thread (its device work on a side
    stream, after this call's kernels) and returns at once: the outputs are final after ``result.wait()``, so a
    stream of calls overlaps one call's host ranking with the next call's search.  Without deferral, a large search
    over a large table runs as ``sub_blocks`` launches over consecutive slices of the active list (default
    :func:`_tie_sub_blocks`), and each slice's tied rows are ranked on the host while the next slice searches.
    ``embedding="matrix"`` (default) embeds with the reference's DCT sequence at range sizes 4, 8 and 16 and an f64
    matrix DCT elsewhere; ``"pocketfft"`` runs scipy's own pocketfft sequence at every supported range size (4 to 49
    and 50, 54, 56, 60, 63, 64: tiles up to 12,799 and a few above), so the embedding, and with it every candidate set
    and match, is the reference's bit for bit there too; ValueError at any other range size.
    ``emb_dim=32`` builds the reference's wide rows (two heads of 16 coefficients, ``res.emb`` f32[nd·32]) and searches
    them through the ``*_dim`` entry points (K ≤ 64: fp16 pre-filter + exact rescoring, fwav_topk_wide.hip); every
    option above works on top, except ``embedding="pocketfft"`` (ValueError) and ``search="f32"`` (ValueError: the
    wide search has one kernel); any other width is NotImplementedError.
    ``query="range"`` (opt-in; the default "domain_row" is the reference's pipeline, quirk Q1) searches with each
    range's own embedding — multi_head_embedding(ranges[i]), what the reference's range_candidates_from_embedding
    computes (fractal.py:337-351), through the same embedding kernel as the pool rows (``embedding`` honoured) — and
    everything after the query vector follows the same contract: the prune, the zero_cand row of an all-zero query,
    scores in the sgemv order of ``blas_threads``, numpy's tie order, the affine solve.  There is no Q9 error then
    (n_ranges > n_domains is legal: the queries do not index the domain table).  ValueError with emb_dim=32 or
    top_k > 64.
    ``fit="clipped"`` (opt-in; the default "reference" is the reference's solve, which picks the slot by the error of
    the unclipped least-squares scale and clips the stored scale afterwards) clips each slot's scale to ±s_clip before
    its offset and error are computed and picks the smallest such error, ties going to the smaller domain index and
    then the unmirrored slot (fwav_affine_fit): ``err`` is then the error of exactly the stored (s, o), s is the
    constrained least-squares scale, and the order of the candidates inside a row cannot change a match.  It sits
    after the search, so it composes with every option above; the whole call — sub-blocks, a shard, the re-solve of
    host-ranked tie rows, deferred or not — solves in the one mode.  The tie check tests the reference's error, so
    ``tie_order="numpy"`` then ranks every K-th place tie on the host, as "numpy_sets" does (stages.tie_mode).
    ``candidates="all"`` (opt-in; the default "embedding" is everything above) picks each range's match among every
    domain of the pool instead of the K that the embedding search proposes (fwav_affine_all): the tuple is what the
    affine solve gives for the candidate row 0 … n_domains − 1 in the call's ``fit``, so it is the best match the pool
    holds — the ceiling that ``top_k``, ``query`` and ``emb_dim`` approach.  The searched ranges are those the energy
    prune keeps (every range without ``fast_mode``); a pruned range gets the tuple the default path gives a pruned
    range (the solve of an all-−1 candidate row).  No query table, zero-query rule, search, tie list or tie check runs,
    so ``top_k``, ``query``, ``emb_dim``, ``embedding``, ``tie_order`` and ``search`` are validated and then unused,
    ``res.cand`` is None and ``n_ties`` = ``n_resolved`` = 0; there is no Q9 error (no query indexes the domain table).
    ``shard``, ``s_clip``, ``fit``, ``on_pool`` and ``events`` (mark "affine_all") work as above.  The cost is
    n_searched · n_domains fits: a second at cfg2 where the default search takes milliseconds.
    """
    if sig.dim() != 1 or sig.dtype != torch.float32 or not sig.is_cuda:
        raise ValueError("compress_device expects a 1-D float32 device tensor")
    dev = sig.device
    st = _stream(dev)
    sig = sig.contiguous()
    n = sig.numel()
    k = int(top_k)
    rs, step = geometry(tile_size)
    if n == 0:
        raise ValueError("a cannot be empty")  # np.convolve on zero frames (fractal.py:895)
    nr = -(-n // rs)
    nd = n_domains_for(n, tile_size, step)
    if k > size_call("fwav_topk_max_k"):
        raise ValueError(f"top_k={k} > {size_call('fwav_topk_max_k')} is not supported by the HIP search")
    check_embedding(embedding, rs)
    dim = check_emb_dim(emb_dim, embedding)
    check_query(query, dim, k)
    stages.check_tie_order(tie_order)
    check_fit(fit)
    all_domains = stages.check_candidates(candidates) == "all"
    threads = _ties.blas_threads() if blas_threads is None else int(blas_threads)
    _mark(events, "voiced_ranges")
    ranges = _voiced_ranges(sig, n, rs, energy_thresh, st)
    partial = torch.empty(1, dtype=torch.float32, device=dev)
    wse = size_call("fwav_weighted_energy_workspace_size", n)
    wsen = torch.empty(wse, dtype=torch.uint8, device=dev)
    call("fwav_weighted_energy", ranges.data_ptr(), n, partial.data_ptr(), wsen.data_ptr(), wse, st)
    _mark(events, "voiced_ranges")
    res = DeviceCompressed(nr, rs, tile_size, step, energy_thresh, n, nd, k, (0, nr), energy_partial=partial,
                           stream=torch.cuda.current_stream(dev))
    if n < tile_size or (nr > nd and query != "range" and not all_domains):
        # the reference returns the empty tuple for silent input before it ever builds domains
        if res.is_silent() or n < tile_size:
            return _empty(n, rs, tile_size, step, energy_thresh, k)
        raise ValueError("mmap length is greater than file size")  # quirk Q9 (fractal.py:1190-1195)
    if search not in ("f16", "f32"):
        raise ValueError("search must be 'f16' (fp16 pre-filter + exact f32 rescoring) or 'f32'")
    if dim != 16 and search != "f16":
        raise ValueError("search='f32' is not available with emb_dim=32 (the wide search has one kernel)")
    if all_domains:  # the embedding is not used: the pool stage in its plainest form (there is no pool-only call)
        embedding, dim, search = "matrix", 16, "f32"
    tab = embed_tables(rs, dev, embedding, dim)
    pool = torch.empty(nd * rs, dtype=torch.float32, device=dev)
    emb = torch.empty(nd * dim, dtype=torch.float32, device=dev)
    emb16 = (torch.empty(stages.emb16_elems(nd, dim), dtype=torch.float16, device=dev) if search == "f16" else None)
    ws_p = size_call("fwav_pool_workspace_size", n, tile_size, rs, step)
    wsp = torch.empty(max(ws_p, 16), dtype=torch.uint8, device=dev)
    _mark(events, "pool_embed")
    stages.pool_embed(sig.data_ptr(), n, tile_size, rs, step, tab.data_ptr(), pool.data_ptr(), emb.data_ptr(),
                      _p(emb16), wsp.data_ptr(), ws_p, st, embedding=embedding, emb_dim=dim)
    _mark(events, "pool_embed")
    if on_pool is not None:
        on_pool(pool)
    if all_domains:
        return _solve_all_domains(res, ranges, pool, shard, energy_thresh, fast_mode, stages.clip32(s_clip), fit, events,
                                  keep_intermediates, st)
    qemb = xq = None
    if query == "range":
        # every range's own embedding, by the pool rows' kernel (the whole signal's: a shard's queries are rows lo … hi)
        _mark(events, "embed_rows")
        qemb = torch.empty(nr * 16, dtype=torch.float32, device=dev)
        qemb16 = (torch.empty(stages.emb16_elems(nr), dtype=torch.float16, device=dev) if emb16 is not None else None)
        stages.embed_rows(ranges.data_ptr(), nr, rs, tab.data_ptr(), qemb.data_ptr(), _p(qemb16), st,
                          embedding=embedding)
        _mark(events, "embed_rows")
        # the first pass seeds range i's limit around the domain whose window starts where the range does
        xq = (qemb, qemb16, nr, rs // step)
    # multi-GPU: bounds chosen from the ranges themselves (fwav.dist balances the prune); evaluated after the pool and
    # embedding kernels are queued, so its host synchronisation overlaps them
    if callable(shard):
        shard = shard(ranges, nr, rs)
    lo, hi = _shard_bounds(shard, nr)
    res.shard = (lo, hi)
    m = hi - lo
    cand = torch.empty(max(m, 1) * k, dtype=torch.int32, device=dev)
    active = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    n_active = torch.empty(1, dtype=torch.int32, device=dev)
    rsh = ranges[lo * rs:hi * rs]
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    s = torch.empty(m, dtype=torch.float32, device=dev)
    o = torch.empty(m, dtype=torch.float32, device=dev)
    sym = torch.empty(m, dtype=torch.uint8, device=dev)
    err = torch.empty(m, dtype=torch.float32, device=dev)
    if m > 0:
        S = _Search(emb, emb16, nd, dim, xq, lo, k, threads, rs, rsh, pool, cand, (idx, s, o, sym, err),
                    stages.clip32(s_clip), stages.tie_mode(tie_order, fit), fit)
        _mark(events, "prune")
        zc = _zero_cand_device(nd, k, dev)
        stages.prune(rsh.data_ptr(), m, lo, rs, stages.prune_thr(energy_thresh), int(bool(fast_mode)), emb.data_ptr(),
                     nd, k, zc.data_ptr(), cand.data_ptr(), active.data_ptr(), n_active.data_ptr(), st, emb_dim=dim,
                     qemb=_p(qemb), n_query_rows=nr)
        _mark(events, "prune")
        nsub = 1
        sliced = False
        if tie_order != "index":
            if sub_blocks is not None:
                nsub = int(sub_blocks)
            elif not defer_ties or nd >= SUB_BLOCK_MIN_DOMAINS:
                nsub = _tie_sub_blocks(m, nd)
            nsub = max(1, min(nsub, m))
            # large tables, deferred: the sliced path too (even as one slice), so that the exact score rows are
            # queued right after the search instead of behind the next call's (the driver thread's side stream
            # would wait for it), and only the copies, numpy's ranking and the fix-up are deferred
            sliced = nsub > 1 or (defer_ties and nd >= SUB_BLOCK_MIN_DOMAINS)
        if not sliced:
            _mark(events, "sim_topk")
            wk = S.workspace_size(m)
            wsk = torch.empty(max(wk, 16), dtype=torch.uint8, device=dev)
            ties = (torch.empty(size_call("fwav_tie_list_size", m), dtype=torch.int32, device=dev)
                    if tie_order != "index" else None)
            S.sim_topk(active.data_ptr(), n_active.data_ptr(), m, ties, wsk, wk, st)
            _mark(events, "sim_topk")
            _mark(events, "affine")
            S.affine(m, st)
            _mark(events, "affine")
        if not sliced and ties is not None:
            # exactly tied scores whose order can change a match: numpy's own ranking for those rows (fwav.ties)
            _mark(events, "ties")
            resolve = torch.empty(m + 1, dtype=torch.int32, device=dev)
            S.tie_check(m, ties, m, resolve, st)

            def counts():
                c = torch.stack([ties[0], resolve[0]]).cpu()
                res.n_ties, res.n_resolved = int(c[0]), int(c[1])
                return resolve[1:1 + res.n_resolved]

            def finish(stream_id):
                rows = counts()
                if res.n_resolved:
                    _ties.resolve_rows(rows, stream=stream_id, **S.rows_kw, **S.fix_kw)

            def stage(stream_id):
                # deferred: on the driver thread, the counts, the exact score rows and their copies; numpy's ranking
                # then runs on the host pool while the driver moves on to the next call, and wait() applies it
                rows = counts()
                if not res.n_resolved:
                    return None
                futs = _ties.rank_rows(_ties.score_row_launches(rows, stream=stream_id, **S.rows_kw), res.n_resolved,
                                       nd, k)
                return rows, futs

            def apply(rows, futs):
                _ties.apply_rows(rows, futs, n_domains=nd, stream=_stream(dev), **S.fix_kw)

            if defer_ties:
                res.apply = apply
                res.pending = _ties.defer(stage, dev)
            else:
                finish(st)
                if keep_intermediates:
                    res.resolved = resolve[1:1 + res.n_resolved]
            _mark(events, "ties")
        elif sliced:
            ties = _search_sub_blocks(S, nsub, m, active, n_active, res, events, st, defer_ties)
    res.pool, res.idx, res.s, res.o, res.sym, res.err, res.n_active = pool, idx, s, o, sym, err, n_active
    if keep_intermediates:
        res.ranges, res.emb, res.cand, res.active, res.qemb = ranges, emb, cand, active, qemb
        if m > 0 and ties is not None:
            res.ties = ties
        if m > 0 and not sliced:
            res.search_ws = wsk
    return res


def _shard_bounds(shard, nr: int) -> tuple[int, int]:
    lo, hi = (0, nr) if shard is None else (int(shard[0]), int(shard[1]))
    if not (0 <= lo <= hi <= nr):
        raise ValueError(f"bad shard {shard} for {nr} ranges")
    return lo, hi


def _solve_all_domains(res: DeviceCompressed, ranges, pool, shard, energy_thresh, fast_mode, s_clip, fit, events,
                       keep_intermediates, st) -> DeviceCompressed:
    """candidates="all": the matches of ranges [lo, hi) among every domain of ``pool``, three launches on the stream
    ``st``: the solve of an all-−1 row for every range (the tuple of a pruned one), the energy prune's list, and
    fwav_affine_all over the listed ranges.  Fills and returns ``res``."""
    dev, nr, rs, nd = ranges.device, res.n_ranges, res.range_size, res.n_domains
    if callable(shard):
        shard = shard(ranges, nr, rs)
    lo, hi = _shard_bounds(shard, nr)
    res.shard = (lo, hi)
    m = hi - lo
    rsh = ranges[lo * rs:hi * rs]
    active = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    n_active = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.float32, device=dev),
            torch.empty(m, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.uint8, device=dev),
            torch.empty(m, dtype=torch.float32, device=dev))
    if m > 0:
        ptrs = [t.data_ptr() for t in outs]
        _mark(events, "prune")
        none = torch.full((m,), -1, dtype=torch.int32, device=dev)
        stages.affine(rsh.data_ptr(), m, rs, none.data_ptr(), 1, pool.data_ptr(), nd, s_clip, ptrs, st, fit=fit)
        stages.prune_energy(rsh.data_ptr(), m, rs, stages.prune_thr(energy_thresh), int(bool(fast_mode)),
                            active.data_ptr(), n_active.data_ptr(), st)
        _mark(events, "prune")
        wn = stages.affine_all_workspace_size(m, nd, rs)
        ws = torch.empty(max(wn, 16), dtype=torch.uint8, device=dev)
        _mark(events, "affine_all")
        stages.affine_all(rsh.data_ptr(), m, rs, active.data_ptr(), n_active.data_ptr(), m, pool.data_ptr(), nd, s_clip,
                          ptrs, ws.data_ptr(), wn, st, fit=fit)
        _mark(events, "affine_all")
    res.pool, res.n_active = pool, n_active
    res.idx, res.s, res.o, res.sym, res.err = outs
    if keep_intermediates:
        res.ranges, res.active = ranges, active
    return res


@dataclasses.dataclass
class _Search:
    """What the search stages of one call share, bound once: the tables (``query``: None, or query="range"'s
    (qemb, qemb16, n_query_rows, seed_stride)), the shard [lo, lo + m) with its ranges, candidates and outputs
    ``outs`` = (idx, s, o, sym, err), ``tie_mode`` = stages.tie_mode(tie_order, fit), and ``fit`` (stages.FITS), the
    mode of every affine solve of the call."""

    emb: torch.Tensor
    emb16: Optional[torch.Tensor]
    nd: int
    dim: int
    query: Optional[tuple]
    lo: int
    k: int
    threads: int
    rs: int
    rsh: torch.Tensor
    pool: torch.Tensor
    cand: torch.Tensor
    outs: tuple
    s_clip: float
    tie_mode: int
    fit: str = "reference"

    @property
    def qemb(self) -> Optional[torch.Tensor]:
        return None if self.query is None else self.query[0]

    @property
    def rows_kw(self) -> dict:
        """The keywords of fwav.ties' exact score rows (score_row_launches, rank_rows_async, resolve_rows)."""
        return dict(emb=self.emb, n_domains=self.nd, q_offset=self.lo, threads=self.threads, emb_dim=self.dim,
                    qemb=self.qemb)

    @property
    def fix_kw(self) -> dict:
        """... and of its fix-up (apply_rows, resolve_rows)."""
        return dict(ranges=self.rsh, range_size=self.rs, pool=self.pool, k=self.k, s_clip=self.s_clip, cand=self.cand,
                    outs=self.outs, fit=self.fit)

    def workspace_size(self, mq: int) -> int:
        return stages.topk_workspace_size(mq, self.nd, self.k, emb_dim=self.dim, f16=self.emb16 is not None)

    def sim_topk(self, active_ptr, n_active_ptr, mq, ties, wsk, wk, st) -> None:
        q = self.query
        stages.sim_topk(self.emb.data_ptr(), _p(self.emb16), self.nd, active_ptr, n_active_ptr, mq, self.lo, self.k,
                        self.threads, self.cand.data_ptr(), _p(ties), wsk.data_ptr(), wk, st, emb_dim=self.dim,
                        query=None if q is None else (q[0].data_ptr(), _p(q[1]), q[2], q[3]))

    def affine(self, m, st) -> None:
        stages.affine(self.rsh.data_ptr(), m, self.rs, self.cand.data_ptr(), self.k, self.pool.data_ptr(), self.nd,
                      self.s_clip, [t.data_ptr() for t in self.outs], st, fit=self.fit)

    def tie_check(self, m, ties, max_ties, resolve, st) -> None:
        stages.tie_check(self.rsh.data_ptr(), m, self.rs, self.cand.data_ptr(), self.k, self.pool.data_ptr(), self.nd,
                         self.emb.data_ptr(), self.lo, self.threads, ties.data_ptr(), max_ties, self.tie_mode,
                         resolve.data_ptr(), st, emb_dim=self.dim, qemb=_p(self.qemb))


#: query sub-blocks of a search whose tied rows are ranked while the next sub-block searches: only where numpy's
#: ranking of a row is expensive (tables of ≥ 4 Mi domains: a cfg3 row 13 ms, a cfg4 row ≈ 50 ms on the host) and
#: every sub-block still fills the chip for a few rounds (≥ 400,000 queries; a slice launch costs ≈ 26 ms more at
#: cfg3, 60 ms at cfg4: profiles/r03/sub_blocks_cfg3.log, sub_blocks_cfg4_eighth.log)
SUB_BLOCK_MIN_DOMAINS = 1 << 22
SUB_BLOCK_QUERIES = 400_000


def _tie_sub_blocks(m: int, nd: int) -> int:
    if nd < SUB_BLOCK_MIN_DOMAINS:
        return 1
    return max(1, min(8, m // SUB_BLOCK_QUERIES))


def _slice_bounds(m: int, nsub: int) -> list[tuple[int, int]]:
    """Consecutive slices [a, b) of m active-list positions, the last one half-size: its tied rows are the only ones
    ranked after the search has ended."""
    nsub = max(1, min(int(nsub), m))
    wts = [2] * (nsub - 1) + [1]
    cuts = [m * sum(wts[:j]) // sum(wts) for j in range(nsub + 1)]
    return [(cuts[j], cuts[j + 1]) for j in range(nsub) if cuts[j + 1] > cuts[j]]


class _Staged:
    """A deferred sliced tie resolution: the slices' (rows, future of their ranking) pairs (DeviceCompressed.wait)."""

    def __init__(self, pend):
        self.pend = pend

    def result(self):
        return (self.pend,)


def _search_sub_blocks(S: _Search, nsub, m, active, n_active, res, events, st, defer=False):
    """The search as ``nsub`` launches over consecutive slices of the active list.  After each slice's search and tie
    check the host reads its tie counts (one synchronisation), queues the exact score rows of its tied rows and hands
    their copies and numpy's ranking to the driver thread (fwav.ties.rank_rows_async); then the next slice searches.
    The affine solve runs once over the shard after the last slice, then the ranked rows are applied.  Returns the
    slices' tie records as one list."""
    dev = S.rsh.device
    bounds = _slice_bounds(m, nsub)
    wk = max(S.workspace_size(b - a) for a, b in bounds)
    wsk = torch.empty(max(wk, 16), dtype=torch.uint8, device=dev)
    pend = []
    lists = []  # each slice's tie records
    n_ties = n_res = 0
    _mark(events, "sim_topk")
    for j0, j1 in bounds:
        mq = j1 - j0
        na = torch.clamp(n_active - j0, 0, mq).to(torch.int32)
        ties = torch.empty(size_call("fwav_tie_list_size", mq), dtype=torch.int32, device=dev)
        S.sim_topk(active[j0:].data_ptr(), na.data_ptr(), mq, ties, wsk, wk, st)
        resolve = torch.empty(mq + 1, dtype=torch.int32, device=dev)
        S.tie_check(m, ties, mq, resolve, st)
        counts = torch.stack([ties[0], resolve[0]]).cpu()
        if _ties._TRACE:
            import time
            print(f"fwav.engine {time.perf_counter():.4f}: slice {j0}..{j1} searched, {int(counts[1])} tied rows",
                  flush=True)
        n_ties += int(counts[0])
        lists.append(ties[1:1 + TIE_REC * int(counts[0])])
        nr_j = int(counts[1])
        n_res += nr_j
        if nr_j:
            rows = resolve[1:1 + nr_j]
            pend.append((rows, _ties.rank_rows_async(rows, k=S.k, stream=st, **S.rows_kw)))
    _mark(events, "sim_topk")
    _mark(events, "affine")
    S.affine(m, st)
    _mark(events, "affine")

    def apply(pend_):
        for rows, fut in pend_:
            _ties.apply_rows(rows, fut.result(), n_domains=S.nd, stream=_stream(dev), **S.fix_kw)

    res.n_ties, res.n_resolved = n_ties, n_res
    res.resolved = torch.cat([r for r, _ in pend]) if pend else torch.empty(0, dtype=torch.int32, device=dev)
    if defer:  # wait() applies the rankings on the caller's stream
        res.pending, res.apply = _Staged(pend), apply
    else:
        _mark(events, "ties")
        apply(pend)
        _mark(events, "ties")
    # one tie list in fwav_sim_topk's layout (count, then the records of every slice)
    return torch.cat([torch.tensor([n_ties], dtype=torch.int32, device=dev)] + lists)


def compact_arrays(idx: torch.Tensor, pool: torch.Tensor, n_domains: int, range_size: int):
    """fwav_compact_domains on ``idx``'s device and current stream: the domain rows that ``idx`` (int32[n_ranges])
    names, in ascending order, and ``idx`` renumbered to them (fractal.py:1278-1322, 1414: the decoder reads
    domains[idx[i]] alone and the file carries its own n_domains).  Returns (idx_out int32[n_ranges], pool_out
    f32[m·rs], kept int32[m], m); when every entry is negative, row 0 is kept (m = 1).  One host synchronisation:
    the 16-byte read of the counts.  IndexError for an entry >= n_domains, as decompress_audio raises it."""
    if idx.dtype != torch.int32 or pool.dtype != torch.float32 or not idx.is_cuda or pool.device != idx.device:
        raise ValueError("compact_arrays expects int32 indices and a float32 pool on one HIP device")
    dev = idx.device
    nr, nd, rs = idx.numel(), int(n_domains), int(range_size)
    if pool.numel() < nd * rs:
        raise ValueError("pool holds fewer than n_domains rows")
    with torch.cuda.device(dev):
        idx, pool = idx.contiguous(), pool.contiguous()
        cap = stages.compact_rows_cap(nd, nr)
        idx_out = torch.empty(nr, dtype=torch.int32, device=dev)
        pool_out = torch.empty(cap * rs, dtype=torch.float32, device=dev)
        kept = torch.empty(cap, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        wsn = size_call("fwav_compact_workspace_size", nd, nr)
        ws = torch.empty(wsn, dtype=torch.uint8, device=dev)
        call("fwav_compact_domains", idx.data_ptr(), nr, pool.data_ptr(), nd, rs, idx_out.data_ptr(),
             pool_out.data_ptr(), kept.data_ptr(), counts.data_ptr(), ws.data_ptr(), wsn, _stream(dev))
        m = stages.compact_count(counts.cpu())
    return idx_out, pool_out[:m * rs], kept[:m], m


def compact_device(res: DeviceCompressed) -> DeviceCompressed:
    """``res`` with its pool cut down to the rows its matches name: ``pool`` f32[m·rs], ``idx`` renumbered,
    ``n_domains`` = m and ``kept`` int32[m], the original index of each kept row (so pool == old pool[kept]); s, o,
    sym and err are the same tensors.  A new result: ``res`` itself is left as it is, and whatever it carries of the
    search (emb, cand, ties) still counts domains in the original numbering.  Waits for a deferred tie resolution
    first (the fix-ups change idx).  ValueError for a shard (its matches do not determine the referenced set: compact
    after the gather); an empty or silent result passes through unchanged."""
    res.wait()
    if tuple(res.shard) != (0, res.n_ranges):
        raise ValueError(f"compact_device needs every range's match: this result is the shard {tuple(res.shard)} of "
                         f"{res.n_ranges} ranges")
    if res.empty or res.n_ranges == 0 or res.is_silent():
        return res
    idx, pool, kept, m = compact_arrays(res.idx, res.pool, res.n_domains, res.range_size)
    return dataclasses.replace(res, idx=idx, pool=pool, kept=kept, n_domains=m)


def decompress_device(idx: torch.Tensor, *args, **kwargs):
    """decompress_audio's loop on ``idx``'s device (made current for the call).  See :func:`_decompress_device`."""
    with torch.cuda.device(idx.device):
        return _decompress_device(idx, *args, **kwargs)


def _decompress_device(idx: torch.Tensor, s: torch.Tensor, o: torch.Tensor, sym: torch.Tensor, pool: torch.Tensor,
                       n_ranges: int, range_size: int, iterations: int = 8, convergence_eps: float = 1e-3,
                       s_clip: float = 16.0, s_damping: float = 0.0):
    """decompress_audio's loop on device.  Returns (recon f32[n_ranges*range_size] tensor, iterations_run,
    deltas f64 list).  One host synchronisation (to read the iteration count and the result buffer), plus one per
    early-exit check: where the f64 Δ cannot decide the reference's Δ < eps (fractal.py:1460-1465), fwav_decode stops
    for fwav_decode_exact (the reference's own sdot order) and the loop resumes when the reference goes on."""
    dev = idx.device
    st = _stream(dev)
    nr, rs = int(n_ranges), int(range_size)
    nd = pool.numel() // rs if rs > 0 else 0
    it = int(iterations)
    eps = float(convergence_eps)
    a = torch.empty(max(nr * rs, 1), dtype=torch.float32, device=dev)
    b = torch.empty(max(nr * rs, 1), dtype=torch.float32, device=dev)
    deltas = torch.zeros(max(it, 1), dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    wsn = size_call("fwav_decode_workspace_size", nr, rs, it)
    ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev)
    kept = []  # the reconstruction a resumed loop starts from

    def snapshot(ptr):
        kept[:] = [(a if ptr == a.data_ptr() else b).clone()]
        return kept[0].data_ptr()

    in_b, done = stages.decode(idx.data_ptr(), s.data_ptr(), o.data_ptr(), sym.data_ptr(), nr, rs, pool.data_ptr(), nd, it,
                               eps, stages.clip32(s_clip), float(s_damping), a.data_ptr(), b.data_ptr(),
                               deltas.data_ptr(), state.data_ptr(), ws.data_ptr(), wsn, st,
                               read_state=lambda: state.cpu().numpy(), snapshot=snapshot)
    out = b if in_b else a
    if nr == 0:
        out = a[:0]
    return out[:nr * rs], done, deltas.cpu().numpy()[:done].tolist()
