"""Inputs of the front-end edge tests (test helper, shared by tests/golden/make_front_edges.py, the CPU pins of
tests/test_front_edges_cpu.py and tests/test_gpu_front_edges.py): the stages before the search — voiced detection and
range formation (fwav_signal.hip), the domain pool and the embedding (fwav_pool_embed.hip).

``embed_rows(rs)``      one table of N_ROWS embedding input rows: the edge rows below (one label each), then random rows.
                        Every row is embedded on its own, so a test may embed any slice, or the table tiled, and
                        compare it with rows of one reference computed once.
``voiced_signal(...)``  a signal whose per-frame level is drawn around the two hysteresis thresholds, so that runs of
                        frames that keep the state are long and lie everywhere.
``pool_signal(...)``    one signal of N_DOMAINS domains at block length bl with a denormal stretch, an overflowing
                        stretch, one inf and one NaN.
``run_signal(...)``     runs of frames at one level each (±level samples, so a frame's energy does not depend on the
                        summation order) — the engineered hysteresis cases of ``scan_cases()``, whose undecided runs
                        span waves, blocks and the trips of the carry kernel (tests/golden/long_scans.npz).

The builders assert on their own inputs only (never on a device's output) that the edges are what they claim."""
import hashlib

import numpy as np

from affine_edges import same_bits_or_nan  # noqa: F401  (bit-equal, any NaN matches any NaN, nothing else relaxed)

F32 = np.float32
N_ROWS = 67

E_SWITCH = tuple(range(-12, -3))                        # b·10^e around both `> 1e-8` normalisation switches
E_SMALL = (-47, -45, -42, -39, -38, -30, -23, -20, -19)  # denormal inputs, denormal or underflowing e·e
E_LARGE = (18, 19, 20, 30, 37)                          # e·e overflows
RANDOM_SCALES = (1e-3, 0.1, 1.0, 1e2)

# the embedding shapes recorded in tests/golden/front_edges.npz, (range size, embedding width): the fixed plans, every
# k_embed_exact instantiation (≤ 16, 24, 32, 48, 64) and every pass kind of the plan (radix 2, 3, 4, 5, the generic
# pass with ido = 1 and ido > 1), and the wide rows (rs 16: ddot_self's 16-value order)
EMBED_FIXED = (4, 8, 16)
EMBED_PLAN = (5, 6, 7, 9, 14, 19, 25, 32, 45, 49, 64)
EMBED_SHAPES = tuple((rs, 16) for rs in EMBED_FIXED + EMBED_PLAN) + tuple((rs, 32) for rs in EMBED_FIXED)
# the matrix path (k_embed<0>), compared with the f64 embedding, not with the fixture
MATRIX_SHAPES = ((5, 16), (7, 16), (19, 16), (33, 16), (65, 16), (100, 16), (19, 32), (33, 32))


def embed_rows(rs, seed=0):
    """→ (rows f32[N_ROWS, rs], names: one label per row).  No row contains −0.0 (a pool built with block length 1
    returns x + 0, which would turn it into +0.0)."""
    rng = np.random.default_rng(7000 + 100 * rs + seed)
    b = rng.normal(0, 0.3, rs)
    rows, names = [], []

    def row(name, v):
        with np.errstate(all="ignore"):
            rows.append(np.asarray(v, np.float64).astype(F32))
        names.append(name)

    sign = np.where(b < 0, -1.0, 1.0)
    row("zero", np.zeros(rs))
    row("constant 0.37", np.full(rs, 0.37))
    row("+-1 alternating", np.where(np.arange(rs) % 2 == 0, 1.0, -1.0))
    imp = np.zeros(rs)
    imp[0] = 1.0
    row("impulse at 0", imp)
    row("impulse at rs-1", imp[::-1])
    row("ramp -1 .. 1", np.linspace(-1.0, 1.0, rs))
    row("1e3 + b*1e-3", 1e3 + b * 1e-3)
    for e in E_SWITCH + E_SMALL + E_LARGE:
        row(f"b*1e{e}", b * 10.0 ** e)
    row("3e38*sign(b)", 3e38 * sign)
    row("constant 3e38", np.full(rs, 3e38))
    row("ramp -3e38 .. 3e38", np.linspace(-3e38, 3e38, rs))
    v = b.copy()
    v[rs // 3] = np.inf
    row("one +inf", v)
    v = b.copy()
    v[rs // 3], v[rs - 1 - rs // 3] = np.inf, -np.inf
    row("+inf and -inf", v)
    for nm, at in (("first", 0), ("middle", rs // 2), ("last", rs - 1)):
        v = b.copy()
        v[at] = np.nan
        row(f"NaN at the {nm} position", v)
    j = 0
    while len(rows) < N_ROWS:
        sc = RANDOM_SCALES[j % len(RANDOM_SCALES)]
        row(f"random, scale {sc:g}", rng.normal(0, 1, rs) * sc)
        j += 1
    out = np.stack(rows) + F32(0.0)   # −0.0 + 0.0 = +0.0 (values that underflowed from a negative b)
    assert out.dtype == F32 and out.shape == (N_ROWS, rs)
    assert not np.any((out == 0) & np.signbit(out))
    return out, names


def matrix_rows(names):
    """The finite, non-overflowing rows of a table (zero, ±1, impulses, ramp, 1e3 + b·1e-3, the random rows): the
    rows the matrix path is held to its accuracy bars on, every one of them."""
    keep = ("zero", "+-1 alternating", "impulse at 0", "impulse at rs-1", "ramp -1 .. 1", "1e3 + b*1e-3")
    return np.array([i for i, nm in enumerate(names) if nm in keep or nm.startswith("random")])


def f64_heads(rows, width):
    """The exactly rounded embedding of fractal.py:154-208 in float64 throughout (the tonal DCT too), unrounded:
    → (tonal f64[n, width/2], transient f64[n, width/2], un-normalised tonal norm f64[n])."""
    import scipy.fftpack
    rows = np.asarray(rows, F32)
    n, rs = rows.shape
    H = width // 2
    w = np.linspace(1.0, 2.0, rs)
    v = scipy.fftpack.dct(rows.astype(np.float64), norm="ortho", axis=-1) * w
    take, tk = min(H, rs - 1), min(H, rs)
    e = np.zeros((n, H))
    e[:, :take] = v[:, 1:1 + take]
    nrm = np.sqrt((e * e).sum(1))
    ok = nrm > 1e-8
    e[ok] /= nrm[ok, None]
    d = np.diff(rows, axis=-1, prepend=rows[:, :1])
    assert d.dtype == F32
    t = np.zeros((n, H))
    t[:, :tk] = scipy.fftpack.dct(d * w, norm="ortho", axis=-1)[:, :tk]
    tn = np.sqrt((t * t).sum(1))
    ok = tn > 1e-8
    t[ok] /= tn[ok, None]
    return e, t, nrm


# ---------------------------------------------------------------------------------------------- voiced detection
VOICED_LEVELS = (0.0, 3e-3, 8e-3, 8.5e-3, 0.02, 0.5)
VOICED_PROBS = (0.15, 0.15, 0.3, 0.2, 0.15, 0.05)
VOICED_THR = 1e-4
VOICED_NF = (1, 2, 3, 4, 5, 6, 64, 65, 1023, 1024, 1025, 2049)
VOICED_FRAMES = (8, 10, 16, 38, 64, 128)     # the GPU sweep; the fixture records FIXTURE_FRAMES
FIXTURE_FRAMES = (8, 38)
TINY_LENGTHS = (1, 2, 3, 5, 7, 9)            # samples, at frame 8: the reflect pad wraps more than once


def voiced_tails(frame):
    return (0, 1, frame - 1)


def voiced_windows(frame):
    return (5, 1) if frame == 8 else (5,)


def voiced_cases(frames):
    """[(frame, nf, tail, smooth_window)] of a sweep over `frames`."""
    return [(f, nf, t, w) for f in frames for w in voiced_windows(f) for nf in VOICED_NF for t in voiced_tails(f)]


def voiced_signal(frame, nf, tail, seed=0):
    """nf frames of level·noise, the level drawn per frame from VOICED_LEVELS; the last frame holds `tail` samples
    (0: the whole frame).  At thresholds 1e-4 / 5e-5 the squares of 8e-3 and 8.5e-3 lie between lo and hi."""
    rng = np.random.default_rng(9000 + 131 * frame + 7 * nf + 1000003 * tail + seed)
    lev = rng.choice(VOICED_LEVELS, size=nf, p=VOICED_PROBS)
    sig = (np.repeat(lev, frame) * rng.normal(0, 1, nf * frame)).astype(F32)
    n = nf * frame if tail == 0 else (nf - 1) * frame + tail
    return np.ascontiguousarray(sig[:n])


# frame lengths at the top of what fwav_voiced_ranges accepts: numpy's pairwise sum of 970, 1022 and 1023 squares
# splits four times before every part is a leaf (1023 → 519 → 263 → 135 → 64 + 71), of 968, 1000 and 1024 three times
LONG_FRAMES = (968, 970, 1000, 1022, 1023, 1024)


def long_frame_signal(frame, seed=0):
    """Two frames: a quiet one, then frame//2 + 1 loud samples whose frame is completed by the reflect pad — the
    second frame's energy is the larger one, so with hi set to it (and lo = 0) the mask says whether the device's
    energy of that frame is above hi."""
    rng = np.random.default_rng(9700 + 3 * frame + seed)
    h = frame // 2
    lev = np.concatenate([np.full(h, 3e-3), np.full(frame - h, 0.01), np.full(h + 1, 0.02)])
    return (lev * rng.normal(0, 1, len(lev))).astype(F32)


def tiny_signal(n):
    rng = np.random.default_rng(9900 + n)
    return rng.normal(0, 0.012, n).astype(F32)


# the threshold-equality cases, (frame, nf, tail) of a recorded signal: the generator sets hi to the smoothed energy
# of one frame and lo to that of another, chosen so that the reference's own mask changes when hi is moved one float
# down or lo one float up — `e > hi` and `e < lo` meet equality and the mask depends on it.  The thresholds are stored
# in the fixture.
EQUAL_CASES = ((8, 65, 0), (8, 1025, 1), (38, 64, 37), (38, 1023, 0))


def sequential_mask(e, hi, lo):
    """fractal.py:900-907 as written: the sequential scan over the smoothed energies, float32 compares."""
    hi, lo = F32(hi), F32(lo)
    out = np.zeros(len(e), np.uint8)
    voiced = False
    for i, v in enumerate(np.asarray(e, F32)):
        if v > hi:
            voiced = True
        elif v < lo:
            voiced = False
        out[i] = voiced
    return out


# ---------------------------------------------------------------------------------------------- domain pool
N_DOMAINS = 70
POOL_CONFIGS = ((4, 1), (5, 2))     # (rs, step): block means of every length; k_domain_pool wherever bl is odd
POOL_BL_FIXTURE = (1, 7, 9, 13, 100, 127, 129, 150, 249, 257, 319)
POOL_BL_SWEEP = tuple(range(1, 320)) + (511, 512, 513, 1023, 1024)
# the first domain that holds the overflowing stretch, the inf and the NaN: domains below P_BIG are finite
P_BIG, P_INF, P_NAN = 35, 40, 55


def pool_signal(bl, rs, step, seed=0):
    """→ (signal f32[n], tile): N_DOMAINS domains of rs blocks of bl samples; tile = rs·bl, plus 1 for odd bl (so
    that tile % rs ≠ 0 is covered: the sample left over is dropped).  Noise at mixed scales with a denormal stretch
    (· 1e-42, at least two whole blocks of the first domains), and near the end, so that the first P_BIG domains stay
    finite, four samples of ±3e38 (sums overflow), one inf and one NaN."""
    rng = np.random.default_rng(5000 + 17 * bl + 1009 * rs + step + seed)
    tile = rs * bl + (bl % 2)
    n = tile + (N_DOMAINS - 1) * step
    scale = np.repeat(rng.choice([1e-3, 0.1, 1.0, 1e2], -(-n // 16)), 16)[:n]
    sig = rng.normal(0, 1, n) * scale
    a, m = 3, max(2 * bl + 2 * step, 8)
    sig[a:a + m] = rng.normal(0, 1, len(sig[a:a + m])) * 1e-42
    last = rs * bl - 1                # the last sample of domain 0 that is used
    p = last + P_BIG * step
    sig[p:p + 4] = 3e38 * np.where(rng.normal(0, 1, 4) < 0, -1.0, 1.0)
    sig[last + P_INF * step] = np.inf
    sig[last + P_NAN * step] = np.nan
    with np.errstate(all="ignore"):
        sig = sig.astype(F32)
    assert len(sig) == n and (n - tile) // step + 1 == N_DOMAINS
    assert np.isfinite(sig[:last + P_BIG * step]).all()
    den = sig[a:a + m]
    assert np.all(np.abs(den) < 1.2e-38) and np.any(den != 0)
    return sig, tile


def numpy_pool(sig, tile, rs, step):
    """build_domains_memmap's arithmetic (fractal.py:301-327) with numpy itself: mean(axis=2, dtype=float32)."""
    bl = tile // rs
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(sig, F32), tile)[::step]
    with np.errstate(all="ignore"):
        return win[:, :bl * rs].reshape(len(win), rs, bl).mean(axis=2, dtype=F32)


# ---------------------------------------------------------------------------------------------- comparisons
def same_or_nan(a, b):
    """same_bits_or_nan for float32, its float64 and float16 counterparts, plain equality for anything else."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == F32:
        return same_bits_or_nan(a, b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {2: np.uint16, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def bad_rows(got, want):
    """Rows of two float32 tables that are not bit-equal (a NaN matches any NaN)."""
    g, w = np.asarray(got, F32), np.asarray(want, F32)
    assert g.shape == w.shape, (g.shape, w.shape)
    ng, nw = np.isnan(g), np.isnan(w)
    ok = (ng == nw) & (ng | (g.view(np.uint32) == w.view(np.uint32)))
    return np.nonzero(~ok.reshape(len(g), -1).all(axis=1))[0].tolist()


def digest(a, dtype="<f4"):
    """SHA-256 of an array's bytes (little-endian, as numpy stores them here)."""
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- fp16 tables
def emb16_tables(emb):
    """The two-part fp16 table of embedding rows emb f32[nd, 16] (fwav_pool_embed.hip store_emb16) in numpy, as
    uint16: hi = f16(x) and, n16/2 further on, lo = f16(x − f32(hi)) — numpy's conversions round to nearest even and
    keep subnormals — each tiled [chunk of 256][half][256][8], rows past nd zero.  Every NaN is made 0x7e00."""
    emb = np.asarray(emb, F32)
    nd = len(emb)
    nc = -(-nd // 256)
    with np.errstate(all="ignore"):
        hi = emb.astype(np.float16)
        lo = (emb - hi.astype(F32)).astype(np.float16)
    parts = []
    for t in (hi, lo):
        full = np.zeros((nc * 256, 16), np.float16)
        full[:nd] = t
        parts.append(np.ascontiguousarray(full.reshape(nc, 256, 2, 8).transpose(0, 2, 1, 3)).reshape(-1))
    return canonical16(np.concatenate(parts))


def canonical16(halfs):
    """fp16 values as uint16 with every NaN made the one quiet NaN 0x7e00 (sign and payload differ between numpy's
    conversion and the device's)."""
    h = np.ascontiguousarray(halfs).view(np.float16)
    u = h.view(np.uint16).copy()
    u[np.isnan(h)] = 0x7E00
    return u


def fp16_special_table(nd, seed=0):
    """Embedding-shaped rows f32[nd, 16], |x| ≤ 1 apart from ±65504, with the values on which an fp16 conversion can
    go wrong written over the first rows: fp16 subnormals (6e-8 … 6e-5, exact and between two of them), exact halfway
    cases between neighbouring fp16 values of both parities (normal and subnormal), values at, just above and below
    half the smallest subnormal (2⁻²⁵), and ±65504."""
    rng = np.random.default_rng(3100 + nd + seed)
    t = rng.uniform(-1, 1, (nd, 16)).astype(F32)
    t *= F32(10.0) ** rng.integers(-6, 1, (nd, 1)).astype(F32)
    sub = np.float16(2.0 ** -24)
    sp = []
    for k in (1, 2, 3, 7, 512, 1000, 1023):                       # subnormals 6e-8 … 6e-5, then between two of them
        sp += [F32(k) * F32(sub), F32(k + 0.5) * F32(sub), F32(k + 0.25) * F32(sub), F32(k + 0.75) * F32(sub)]
    for h in (np.float16(0.1), np.float16(0.333), np.float16(1.0) - np.float16(2.0 ** -10), np.float16(6.1e-5),
              np.float16(2.0 ** -14), np.float16(0.5)):           # halfway to the next fp16 value, both parities
        for v in (h, np.nextafter(h, np.float16(2))):
            nx = np.nextafter(v, np.float16(2))
            mid = (F32(v) + F32(nx)) / F32(2)
            sp += [mid, np.nextafter(mid, F32(2)), np.nextafter(mid, F32(0))]
    half_sub = F32(2.0 ** -25)
    sp += [half_sub, np.nextafter(half_sub, F32(1)), np.nextafter(half_sub, F32(0)), F32(2.0 ** -26), F32(1e-30),
           F32(1e-45), F32(65504), F32(0)]
    sp = np.array(sp, F32)
    sp = np.concatenate([sp, -sp])
    m = min(len(sp), t.size)
    t.reshape(-1)[:m] = sp[:m]
    return t


# ---------------------------------------------------------------------------------------------- engineered runs
# The sequential part of the hysteresis (fwav_signal.hip): a frame's state is the decision of the last decisive frame
# before it, found by a max-scan over threads (SCAN_THREAD frames each), waves (SCAN_WAVE frames) and blocks
# (SCAN_BLOCK frames) in k_frame_state, and over the blocks' last decisions in k_voiced_carry, one workgroup that
# takes CARRY_TRIP blocks per loop trip, CARRY_WAVE per wave.  voiced_signal's undecided runs are a handful of frames
# long; these signals hold runs of whole waves, blocks and trips.
A_KEEP, A_LOUD, A_QUIET = 8.5e-3, 0.02, 1e-3    # a² between lo and hi at 1e-4 / 5e-5, above hi, below lo
SCAN_THREAD, SCAN_WAVE, SCAN_BLOCK = 4, 256, 1024
CARRY_WAVE, CARRY_TRIP = 64, 1024
SCAN_WINDOWS = (5, 1)
IN_BLOCK_P = (0, 3, 4, 255, 256, 257, 1023, 1024, 1025)
IN_BLOCK_L = (1, 4, 255, 256, 257, 768, 1024, 2048, 3 * 1024 + 5)
WAVE_BLOCKS = (65, 66, 130)
TRIP_BLOCKS = (1025, 1026, 2049)
WAVE_FRAMES = (8, 38, 64)      # the wave list runs at frames 38 (range size 19: the runtime-rs kernels) and 64 too
DECISION_AT = 500              # a decision placed "in block b" sits at frame b·1024 + 500


def run_signal(frame, runs, seed=0, tail=0):
    """runs = [(level, n_frames), …] → samples ±level with seeded random signs, so that a frame's energy is level²
    whatever the order of its sum; the last frame holds `tail` samples (0: the whole frame)."""
    lev = np.repeat(np.array([l for l, _ in runs], F32), [n for _, n in runs])
    nf = len(lev)
    rng = np.random.default_rng(12000 + seed)
    sig = np.repeat(lev, frame)
    np.negative(sig, out=sig, where=rng.integers(0, 2, nf * frame, dtype=np.uint8).astype(bool))
    n = nf * frame if tail == 0 else (nf - 1) * frame + tail
    assert sig.dtype == F32 and 0 < n <= len(sig)
    return np.ascontiguousarray(sig[:n])


def decision_frames(window):
    """Frames at A_QUIET or A_LOUD that make a decision: with the 5-tap smoothing one quiet frame among A_KEEP frames
    is not decisive ((4·7.2e-5 + 1e-6)/5 > lo), three are — and one loud frame is not where the window is cut short
    (two frames in all: (4e-4 + 7.2e-5)/5 < hi), three are; without smoothing one is, exactly where it is put."""
    return 3 if window > 1 else 1


class ScanCase:
    """One engineered signal: `runs` for run_signal at `frame`, detected with `window`; `need` = the least counts of
    scan_profile() the case is there for (asserted on the oracle's smoothed energies before a device is touched)."""

    def __init__(self, name, frame, window, runs, need, seed=0, tail=0):
        self.name, self.frame, self.window, self.runs = name, frame, window, tuple(runs)
        self.need, self.seed, self.tail = dict(need), seed, tail
        self.nf = sum(n for _, n in self.runs)

    def signal(self):
        return run_signal(self.frame, self.runs, self.seed, self.tail)

    def __repr__(self):
        return self.name


def scan_claims(case):
    """[(first frame, last frame + 1, state)] of the A_KEEP runs: the state their undecided frames must come out
    with — that of the run before (loud: voiced, quiet or silent: unvoiced), unvoiced before any decision."""
    out, at, state = [], 0, 0
    for lev, n in case.runs:
        if lev == A_KEEP:
            out.append((at, at + n, state))
        else:
            state = 1 if lev > A_KEEP else 0
        at += n
    return out


def scan_profile(e, hi=VOICED_THR, lo=VOICED_THR * 0.5):
    """What the scans of a signal with smoothed frame energies `e` have to carry, in numpy:
      decisive          frames above hi or below lo
      carried_threads   4-frame groups without a decision, after a decision in the same 256-frame wave
      carried_waves     whole 256-frame waves without a decision, after a decisive wave of the same block (wlast = −1)
      undecided_blocks  1024-frame blocks without a decision (blast = −1)
      leading_blocks    blocks that start undecided with no decision before them (carry = −1: unvoiced)
      far_blocks        blocks that start undecided and whose last decision lies further back than the block before
      wave_crossings    … lies in another 64-block wave of k_voiced_carry
      trip_crossings    … lies in another 1024-block trip of k_voiced_carry's loop
      trip_skips        … lies two or more trips back (a trip without any decision hands it on)
    and `src`, per block the block that holds the last decision before it (−1: none)."""
    e = np.asarray(e, F32)
    nf = len(e)
    dec = (e > F32(hi)) | (e < F32(lo))
    last = np.maximum.accumulate(np.where(dec, np.arange(nf), -1))      # the last decisive frame ≤ f
    before = np.concatenate([[-1], last[:-1]])                          # … < f

    def groups(size):
        first = np.arange(0, nf, size)
        return first, np.add.reduceat(dec.astype(np.int64), first) == 0

    tf, tnone = groups(SCAN_THREAD)
    wf, wnone = groups(SCAN_WAVE)
    bf, bnone = groups(SCAN_BLOCK)
    b = np.arange(len(bf))
    src = np.where(before[bf] >= 0, before[bf] // SCAN_BLOCK, -1)
    used = ~dec[bf] & (src >= 0)
    prof = dict(
        decisive=int(dec.sum()),
        carried_threads=int((tnone & (before[tf] >= tf // SCAN_WAVE * SCAN_WAVE) & (tf % SCAN_WAVE != 0)).sum()),
        carried_waves=int((wnone & (before[wf] >= wf // SCAN_BLOCK * SCAN_BLOCK) & (wf % SCAN_BLOCK != 0)).sum()),
        undecided_blocks=int(bnone.sum()),
        leading_blocks=int((~dec[bf] & (src < 0)).sum()),
        far_blocks=int((used & (src < b - 1)).sum()),
        wave_crossings=int((used & (src // CARRY_WAVE < b // CARRY_WAVE)).sum()),
        trip_crossings=int((used & (src // CARRY_TRIP < b // CARRY_TRIP)).sum()),
        trip_skips=int((used & (b // CARRY_TRIP - src // CARRY_TRIP >= 2)).sum()))
    return prof, src


def in_block_cases(window):
    """One decision at frame p, then an undecided run of L frames, p and L around a thread's 4 frames, a wave's 256
    and the block's 1024 — voiced: A_KEEP frames (unvoiced: nothing decided yet), one loud frame, the run, which comes
    out voiced; unvoiced: a loud block first, A_KEEP frames (voiced), the quiet decision at 1024 + p, the run, which
    comes out unvoiced.  Then the leading run: more than two blocks with nothing decided, then a loud frame."""
    q = decision_frames(window)
    out = []
    for p in IN_BLOCK_P:
        for L in IN_BLOCK_L:
            need = {}
            if L >= 2 * SCAN_BLOCK:             # any 2047 consecutive frames hold a whole block
                need["undecided_blocks"] = 1
            if L >= 3 * SCAN_BLOCK:             # … any 3071 two in a row: the second one's carry skips the first
                need["far_blocks"] = 1
            lead = [(A_KEEP, p)] if p else []
            out.append(ScanCase(f"inblock_w{window}_voiced_p{p}_L{L}", 8, window, lead + [(A_LOUD, q), (A_KEEP, L)],
                                need, seed=len(out)))
            out.append(ScanCase(f"inblock_w{window}_unvoiced_p{p}_L{L}", 8, window,
                                [(A_LOUD, SCAN_BLOCK)] + lead + [(A_QUIET, q), (A_KEEP, L)], need, seed=len(out),
                                tail=5 if L % 2 else 0))
    # with the 5-tap smoothing frame 0 (a window of three) is below lo: a decision, so the blocks are not "leading"
    need = dict(leading_blocks=3) if window == 1 else dict(far_blocks=1, undecided_blocks=1)
    out.append(ScanCase(f"inblock_w{window}_leading", 8, window,
                        [(A_KEEP, 2 * SCAN_BLOCK + 300), (A_LOUD, q), (A_KEEP, 10)], need, seed=len(out)))
    return out


def carry_runs(nb, decisions, window):
    """nb blocks of A_KEEP frames with one decision per (block, "loud" | "quiet") at frame block·1024 + 500."""
    runs, at = [], 0
    for blk, kind in decisions:
        f = blk * SCAN_BLOCK + DECISION_AT
        runs.append((A_KEEP, f - at))
        n = decision_frames(window)
        runs.append((A_LOUD if kind == "loud" else A_QUIET, n))
        at = f + n
    runs.append((A_KEEP, nb * SCAN_BLOCK - at))
    return runs


def wave_cases(frame, window):
    """k_voiced_carry's waves: 65, 66 and 130 blocks with the only decision in block 0, in block 63 (the last lane of
    the carry's first wave), in block 64 (the first of its second), and a voiced decision in block 0 with an unvoiced
    one in block 64."""
    out = []
    w1 = window == 1
    for nb in WAVE_BLOCKS:
        pats = (("only0", [(0, "loud")], dict(wave_crossings=nb - 64, far_blocks=nb - 2, undecided_blocks=nb - 2)),
                ("only63", [(63, "loud")], dict(wave_crossings=nb - 64, undecided_blocks=nb - 3,
                                               **(dict(leading_blocks=64) if w1 else dict(far_blocks=62)))),
                ("only64", [(64, "loud")], dict(undecided_blocks=nb - 3,
                                               **(dict(leading_blocks=65) if w1 else dict(wave_crossings=1)))),
                ("v0_u64", [(0, "loud"), (64, "quiet")], dict(wave_crossings=1, far_blocks=62,
                                                              undecided_blocks=nb - 3)))
        for nm, decisions, need in pats:
            out.append(ScanCase(f"wave_f{frame}_w{window}_{nb}_{nm}", frame, window, carry_runs(nb, decisions, window),
                                need, seed=100 + len(out), tail=3 if nb % 2 else 0))
    return out


def trip_cases(window):
    """k_voiced_carry's loop: 1025, 1026 and 2049 blocks (the largest 2049·1024·8 samples) with the only decision in
    block 0; a voiced decision in block 0 and an unvoiced one in block 1023 (the last of trip 1) or 1024 (the first of
    trip 2); the only decision, a voiced one, in block 1023 (a `running` that restarted at −1 gives the same mask as
    an unvoiced decision, so the state handed over is the voiced one too); and, where there is a third trip (2049
    blocks), an unvoiced decision in block 0 and a voiced one in block 700 that a decision-free trip 2 hands on to
    trip 3."""
    out = []
    for nb in TRIP_BLOCKS:
        pats = [("only0", [(0, "loud")], dict(trip_crossings=nb - 1024, **(dict(trip_skips=1) if nb > 2048 else {}))),
                ("v0_u1023", [(0, "loud"), (1023, "quiet")], dict(trip_crossings=1, far_blocks=1021)),
                ("v0_u1024", [(0, "loud"), (1024, "quiet")], dict(trip_crossings=1, far_blocks=1022)),
                ("only1023", [(1023, "loud")], dict(trip_crossings=nb - 1024, undecided_blocks=nb - 3))]
        if nb > 2 * CARRY_TRIP:
            pats.append(("u0_v700_skip", [(0, "quiet"), (700, "loud")], dict(trip_skips=1, trip_crossings=1025)))
        for nm, decisions, need in pats:
            out.append(ScanCase(f"trip_w{window}_{nb}_{nm}", 8, window, carry_runs(nb, decisions, window), need,
                                seed=200 + len(out), tail=3 if nb % 2 else 0))
    return out


def scan_lists():
    """name → [ScanCase]: the in-block, wave and trip lists at frame 8 with smooth_window 5 and 1 (where a decisive
    frame sits exactly where it is put), and the wave list at frames 38 and 64 (window 5)."""
    out = {}
    for w in SCAN_WINDOWS:
        out[f"inblock_w{w}"] = in_block_cases(w)
    for f in WAVE_FRAMES:
        for w in (SCAN_WINDOWS if f == 8 else (5,)):
            out[f"wave_f{f}_w{w}"] = wave_cases(f, w)
    for w in SCAN_WINDOWS:
        out[f"trip_w{w}"] = trip_cases(w)
    return out


def scan_cases():
    return [c for lst in scan_lists().values() for c in lst]


# through engine.compress_device (tile 1024: range size 4, frame 8, window 5): a loud start, three whole blocks of
# A_KEEP frames and more (voiced), then silence
PRODUCT_TILE = 1024
PRODUCT_CASE = ScanCase("product_3_blocks_then_silence", 8, 5,
                        [(A_LOUD, 8), (A_KEEP, 4 * SCAN_BLOCK), (0.0, SCAN_BLOCK + 90)],
                        dict(undecided_blocks=3, far_blocks=2), seed=300, tail=3)


def mask_runs(frame_mask):
    """A per-frame mask as run lengths → (first value, the frames at which the value changes)."""
    m = np.asarray(frame_mask, np.uint8)
    return int(m[0]), np.nonzero(m[1:] != m[:-1])[0].astype(np.int64) + 1


def mask_from_runs(first, changes, nf):
    """… and back: u8[nf]."""
    flips = np.zeros(nf, np.int64)
    flips[np.asarray(changes, np.int64)] = 1
    return ((first + np.cumsum(flips)) & 1).astype(np.uint8)
