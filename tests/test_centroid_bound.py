"""The centroid pre-filter's threshold (csrc/fwav_centroid_bound.h) against a float64 brute force.

tests/centroid_bound/bound_check.cpp includes the header the kernel includes and is built with the host compiler under
UBSan.  For centroids of fp16 members (unit-norm heads and shorter, identical members, a zero head, all-zero vectors,
members 1e-3 … 0.5 apart) and fp16 table rows (random ones, and rows built to maximise the bound,
d_h = a ĉ_h + √(1 − a²) ê⊥_h over a grid of a), no tolerance:

  every row with s16(c, d) ≤ thc has s16(q_m, d) < t_min − 4e-6 for every member (finite t_min; < t_min otherwise)

— the kernel skips a tile for a centroid exactly where every row has s16(c, d) ≤ thc, and 4e-6 is the share of the
rounding allowance η = 1e-5 that the two MFMA accumulations may use (2 × 16 roundings of 2⁻²⁴ · 2), which float64
scores do not spend.  The fallback cases return exactly the worst-case threshold t_min − ((ρ_0 + ρ_1)(1 + 2⁻⁹) + 1e-5)
of f32 arithmetic.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-compression_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "centroid_bound", "bound_check.cpp")
OUT = os.path.join(CSRC, "build", "centroid_bound")
TMINS = [-np.inf, -1.0, 0.0, 0.5, 1.0, 1.5, 1.75, 1.9, 1.95, 1.99, 2.0, 2.01, np.inf]
MFMA_SHARE = 4e-6

f32 = np.float32


def _compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return [c]
    return ["hipcc", "-x", "c++"]  # the HIP compiler as a host C++ compiler (no offload)


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"bound_check.{os.getpid()}")
    subprocess.check_call([*_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, DRIVER, "-o", path])
    yield path
    os.remove(path)


def _fp16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _unit_heads(rng, n, norms=(1.0, 1.0)):
    v = rng.standard_normal((n, 2, 8))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    return v * np.asarray(norms, np.float64)[None, :, None]


def _centroid(members):
    """The kernel's centroid: the f32 sum of the members in order, divided by their number, rounded to fp16."""
    s = np.zeros(16, f32)
    for m in members:
        s = (s + m.astype(f32)).astype(f32)
    return (s / f32(len(members))).astype(np.float16).astype(np.float64)


def _near(rng, q, dist, norms):
    """A vector at about `dist` from q with the same head norms."""
    v = q.reshape(2, 8) + dist * _unit_heads(rng, 1)[0] / np.sqrt(2.0)
    n = np.linalg.norm(v, axis=1, keepdims=True)
    return (v / np.where(n > 0, n, 1.0) * np.asarray(norms)[:, None]).reshape(16)


def _cases():
    rng = np.random.default_rng(20240607)
    out = []
    for norms in ((1.0, 1.0), (1.0, 0.6), (0.3, 0.9), (0.05, 0.02)):
        for dist in (1e-3, 3e-3, 1e-2, 0.05, 0.1, 0.25, 0.5):
            for nm in (2, 2, 4):
                q0 = _unit_heads(rng, 1, norms)[0].reshape(16)
                ms = [q0] + [_near(rng, q0, dist, norms) for _ in range(nm - 1)]
                out.append((f"norms{norms} dist{dist} nm{nm}", [_fp16(m) for m in ms]))
    q = _fp16(_unit_heads(rng, 1)[0].reshape(16))
    out.append(("identical", [q, q.copy()]))
    out.append(("single", [q]))
    z = q.copy()
    z[8:] = 0.0
    out.append(("zero head both", [z, _fp16(np.concatenate([_near(rng, q, 0.05, (1, 1))[:8], np.zeros(8)]))]))
    out.append(("zero head one", [z, q]))
    out.append(("opposite heads", [z, np.concatenate([np.zeros(8), q[8:]])]))  # n_h > 0 in both, e ∥ c
    out.append(("antipodal", [q, -q]))                                          # the centroid is all zero
    out.append(("all zero", [np.zeros(16), np.zeros(16)]))
    out.append(("zero and unit", [np.zeros(16), q]))
    tiny = np.zeros(16)
    tiny[3] = 2.0 ** -24  # an fp16 subnormal
    out.append(("subnormal", [tiny, 2 * tiny]))
    out.append(("subnormal and unit", [tiny, q]))
    return out


def _rows(rng, c, members):
    """fp16 table rows: random heads of norm ≤ 1, and d_h = a ĉ_h + √(1 − a²) ê⊥_h for every member's e⊥ (both signs,
    a grid of a per head) — the rows that make the bound's inequalities tight."""
    rows = [(_unit_heads(rng, 1500) * rng.random((1500, 2, 1)) ** 0.25).reshape(-1, 16)]
    near = c.reshape(2, 8) / np.maximum(np.linalg.norm(c.reshape(2, 8), axis=1, keepdims=True), 1e-30)
    rows.append((near[None] + 0.1 * rng.standard_normal((500, 2, 8))).reshape(-1, 16))
    rows[-1] = (rows[-1].reshape(-1, 2, 8)
                / np.maximum(np.linalg.norm(rows[-1].reshape(-1, 2, 8), axis=2, keepdims=True), 1.0)).reshape(-1, 16)
    grid = np.concatenate([np.linspace(-1, 1, 9), 1 - np.geomspace(1e-4, 0.3, 8)])
    A0, A1 = [g.reshape(-1) for g in np.meshgrid(grid, grid)]
    ch = c.reshape(2, 8)
    for m in members:
        e = (m - c).reshape(2, 8)
        u, w = np.zeros((2, 8)), np.zeros((2, 8))
        for h in range(2):
            n = np.linalg.norm(ch[h])
            if n > 0:
                u[h] = ch[h] / n
            p = e[h] - (e[h] @ u[h]) * u[h]
            if np.linalg.norm(p) > 0:
                w[h] = p / np.linalg.norm(p)
            elif n == 0 and np.linalg.norm(e[h]) > 0:
                w[h] = e[h] / np.linalg.norm(e[h])
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                d0 = A0[:, None] * u[0] + s0 * np.sqrt(1 - A0 ** 2)[:, None] * w[0]
                d1 = A1[:, None] * u[1] + s1 * np.sqrt(1 - A1 ** 2)[:, None] * w[1]
                rows.append(np.concatenate([d0, d1], axis=1))
    r = np.concatenate(rows).reshape(-1, 2, 8)
    r = _fp16((r / np.maximum(np.linalg.norm(r, axis=2, keepdims=True), 1.0)).reshape(-1, 16))
    assert np.linalg.norm(r.reshape(-1, 2, 8), axis=2).max() <= 1 + 2.0 ** -9  # D of the header
    return r


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float64).reshape(-1))


def _run(exe, cases, tmins):
    text = "".join(f"{len(ms)} {_hex(_centroid(ms))} {_hex(np.stack(ms))} {len(tmins)} {_hex(tmins)}\n"
                   for _, ms in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24"))
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    v = np.array([[float.fromhex(x) for x in ln.split()] for ln in r.stdout.split("\n") if ln], np.float64)
    return v.reshape(len(cases), len(tmins), 2)


def _old_threshold(c, members, tmin):
    """t_min − ((ρ_0 + ρ_1)(1 + 2⁻⁹) + 1e-5) as f32 arithmetic evaluates it (sums in index order)."""
    rho = [f32(0), f32(0)]
    for m in members:
        for h in range(2):
            d2 = f32(0)
            for i in range(8):
                d = f32(m[8 * h + i]) - f32(c[8 * h + i])
                d2 = f32(d2 + f32(d * d))
            rho[h] = max(rho[h], np.sqrt(d2, dtype=f32))
    slack = f32(f32(f32(rho[0] + rho[1]) * f32(1 + 2.0 ** -9)) + f32(1e-5))
    with np.errstate(invalid="ignore"):
        return f32(f32(tmin) - slack)


@pytest.fixture(scope="module")
def results(exe):
    cases = _cases()
    return cases, _run(exe, cases, TMINS)


def test_no_row_below_the_threshold_reaches_a_member_limit(results):
    cases, thc = results
    rng = np.random.default_rng(7)
    checked = tighter = 0
    for (name, ms), th in zip(cases, thc):
        c = _centroid(ms)
        rows = _rows(rng, c, ms)
        sc = rows @ c
        sm = rows @ np.stack(ms).T
        for t, (tight, old) in zip(TMINS, th):
            assert tight >= old or (np.isnan(tight) and np.isnan(old)), (name, t, tight, old)
            tighter += tight > old
            lim = t - MFMA_SHARE if np.isfinite(t) else t
            for nm, v in (("tight", tight), ("old", old)):
                below = sc <= v
                checked += int(below.sum())
                if below.any():
                    worst = sm[below].max()
                    assert worst < lim, (name, nm, t, v, worst)
    assert checked > 100000 and tighter > 100  # the condition was exercised, and the new bound does cut further


def test_fallback_cases_return_the_worst_case_threshold(results):
    cases, thc = results
    n = 0
    for (name, ms), th in zip(cases, thc):
        c = _centroid(ms)
        for t, (tight, old) in zip(TMINS, th):
            want = np.float64(_old_threshold(c, ms, t))
            assert old == want or (np.isnan(old) and np.isnan(want)), (name, t, old, want)
            if not np.isfinite(t) or t <= 0.0 or not c.any():  # cold, −∞ or +∞ limits; an all-zero centroid
                assert tight == want or (np.isnan(tight) and np.isnan(want)), (name, t, tight, want)
                n += 1
    assert n >= 4 * len(cases)


def test_tighter_where_the_filter_decides(results):
    """Unit-norm members 0.05 … 0.25 apart at limits 1.75 … 1.95 (cfg2's floor and K-th scores): the score-dependent
    bound gives the higher threshold."""
    cases, thc = results
    n = 0
    for (name, ms), th in zip(cases, thc):
        if not name.startswith("norms(1.0, 1.0)") or not any(f"dist{d} " in name for d in (0.05, 0.1, 0.25)):
            continue
        for t, (tight, old) in zip(TMINS, th):
            if 1.75 <= t <= 1.95:
                assert tight > old, (name, t, tight, old)
                n += 1
    assert n >= 9
