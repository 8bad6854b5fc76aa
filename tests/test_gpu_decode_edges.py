"""GPU decode (fwav_decode.hip) on the edge table of tests/decode_edges.py, against the reference's own recorded
outputs (tests/golden/decode_edges.npz) and against O.decode (pinned to that fixture by
tests/test_oracle_golden.py::test_decode_edges_pinned): range sizes 1 … 1024 (the short branch of pw_reg, every
resident bucket, the streaming kernels with one and with several pairwise leaves), row counts below one block and one
off the thread-group boundaries, sentinel indices other than −1, constant and tiny tiles, den on both sides of 1e-12,
−0.0, s far outside s_clip, sym bytes 2 and 255, NaN / inf / ±3e38 in tiles, s and o, the whole table × 1e-20, × 1e-30
and × 1e19 (Δ sums in float32's denormal and overflow range: the exact check decides), and the twelve parameter sets
of decode_edges.PARAMS (s_damping 1e-6, 1 and 1.5, s_clip 0, −16 and inf, 2 and 3 iterations with eps > 0).

Bar: every reconstruction bit-equal, except that a NaN matches any NaN; the same iteration count; every Δ by
decode_edges.same_delta (the reference's own value where the exact check decided, else the oracle's float64 measure
to 1e-12 relative, NaN with NaN).  No case and no row is skipped."""
import json
import os

import numpy as np
import pytest

import decode_edges as DE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import dist, engine  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

RS_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 127, 128, 129, 130, 300, 1024)
ROW_COUNTS = {rs: (1, 3, 255, 257, 511, 513, 1023, 1025, 4095, 4096, 4097, 8193) for rs in (4, 5, 8, 16, 20, 32)}
ROW_COUNTS[40] = (1, 255, 256, 257, 1025)
N_TABLE = 8193


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


class Table:
    """One built table on the host and on the device; decode(n, …) runs the device on its first n rows alone."""

    def __init__(self, rs, nr, kind):
        self.rs, self.nr, self.kind = rs, nr, kind
        self.idx, self.s, self.o, self.sym, self.pool, names = DE.build(rs, nr, kind)
        self.label = DE.labels(names, nr)
        self.dev = [td(self.idx), td(self.s), td(self.o), td(self.sym), td(self.pool.reshape(-1))]

    def host(self, n=None):
        n = self.nr if n is None else n
        return self.idx[:n], self.s[:n], self.o[:n], self.sym[:n], self.pool, n, self.rs

    def decode(self, n=None, **kw):
        n = self.nr if n is None else n
        rec, ran, deltas = engine.decompress_device(*self.dev, n, self.rs, **kw)
        return rec.cpu().numpy(), ran, deltas

    def oracle(self, n=None, **kw):
        """→ (recon, iterations, [(f64 Δ, reference Δ, Σ rec², Σ diff²)])."""
        with np.errstate(all="ignore"):
            return O.decode(*self.host(n), deltas="sums", **kw)


def bad_rows(got, want, n, rs):
    """Rows of two reconstructions that are not bit-equal (a NaN matches any NaN)."""
    g, w = np.asarray(got, np.float32).reshape(n, rs), np.asarray(want, np.float32).reshape(n, rs)
    ng, nw = np.isnan(g), np.isnan(w)
    ok = (ng == nw) & (ng | (g.view(np.uint32) == w.view(np.uint32)))
    return np.nonzero(~ok.all(axis=1))[0].tolist()


def same(a, b):
    return a == b or (a != a and b != b)


def check_against_oracle(tb, got, want, n, where):
    rec, ran, deltas = got
    ref, it, sums = want
    assert len(rec) == n * tb.rs
    bad = bad_rows(rec, ref, n, tb.rs)
    assert not bad, (f"{where}: rows " + str([(r, tb.label[r], rec.reshape(n, -1)[r][:4], ref.reshape(n, -1)[r][:4])
                                              for r in bad[:5]]))
    assert ran == it, (where, ran, it)
    assert len(deltas) == len(sums)
    for t, (a, q) in enumerate(zip(deltas, sums)):
        assert DE.same_delta(a, q[0], q[1]), (where, t, a, q)


def checked_iterations(sums, n_values, eps):
    """The iterations of an oracle run at which the device must take the exact check (fwav.dist.decode_decision, the
    host's statement of dec_decide), and those among them whose sums are in float32's denormal or overflow range."""
    beta = dist.decode_beta(n_values)
    chk = [t for t, (d64, _, rr, dd) in enumerate(sums) if dist.decode_decision(rr, dd, d64, eps, beta) == 2]
    ext = [t for t in chk if sums[t][3] < 1e-30 or sums[t][3] > 1e36 or (sums[t][2] > 0 and (
        sums[t][2] < 1e-30 or sums[t][2] > 1e36))]
    return chk, ext


@pytest.mark.parametrize("rs", DE.FIXTURE_RS)
def test_device_equals_the_reference_fixture(rs):
    """engine.decompress_device on every recorded entry against the reference's own decompress_audio: reconstruction
    (per-row digests, and the rows themselves where the fixture keeps them), iteration count, and every Δ as the log
    prints it."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "decode_edges.npz"))
    meta = json.loads(str(fx["params"]))
    nr = meta["nr"]
    tables = {}
    n_seen = 0
    for e_rs, kind, pi in (tuple(e) for e in meta["entries"]):
        if e_rs != rs:
            continue
        n_seen += 1
        if kind not in tables:
            tables[kind] = Table(rs, nr, kind)
            assert DE.input_digest(*tables[kind].host()[:5]) == meta["inputs"][f"rs{rs}_{kind}"]
        tb = tables[kind]
        tag = f"rs{rs}_{kind}_p{pi}"
        kw = DE.kw(DE.PARAMS[pi])
        rec, ran, deltas = tb.decode(**kw)
        _, _, sums = tb.oracle(**kw)
        dig = DE.row_digests(rec, nr, rs)
        bad = [r for r in range(nr) if not np.array_equal(dig[r], fx[f"dig_{tag}"][r])]
        assert not bad, f"{tag}: rows {[(r, tb.label[r], rec.reshape(nr, rs)[r][:4]) for r in bad[:8]]}"
        if f"rec_{tag}" in fx:
            assert DE.same_bits_or_nan(rec, fx[f"rec_{tag}"]), tag
        assert ran == int(fx[f"it_{tag}"]), (tag, ran, int(fx[f"it_{tag}"]))
        want = fx[f"dl_{tag}"].tolist()
        assert len(deltas) == len(want) == len(sums)
        for t, (a, q, w) in enumerate(zip(deltas, sums, want)):
            assert DE.same_delta(a, q[0], q[1]), (tag, t, a, q)
            assert DE.same_delta(DE.fmt_delta(a), DE.fmt_delta(q[0]), w), (tag, t, a, q, w)
    assert n_seen == len(DE.KINDS) * len(DE.FIXTURE_SETS_ALL_KINDS) + len(DE.PARAMS) - len(DE.FIXTURE_SETS_ALL_KINDS)


@pytest.mark.parametrize("rs", RS_SWEEP)
def test_sweep_against_oracle(rs):
    """Every kind × every parameter set at this range size against O.decode."""
    nr = 67 if rs >= 128 else 300
    for kind in DE.KINDS:
        tb = Table(rs, nr, kind)
        for pi, p in enumerate(DE.PARAMS):
            kw = DE.kw(p)
            check_against_oracle(tb, tb.decode(**kw), tb.oracle(**kw), nr, f"rs={rs} {kind} set {pi + 1}")


@pytest.mark.parametrize("rs", sorted(ROW_COUNTS))
def test_row_counts(rs):
    """The first nr rows of one 8193-row table decoded alone — below one block (4096 ranges), on and one off the
    thread-group boundaries (256, 512, 1024 ranges), one past a block: the same rows of one oracle decode of the whole
    table (eps = 0: a range depends on its own row alone), and the Δ values of an oracle decode of the slice."""
    kw = dict(iterations=5, convergence_eps=0.0)
    for kind in ("finite", "nonfinite"):
        tb = Table(rs, N_TABLE, kind)
        whole, it, _ = tb.oracle(**kw)
        assert it == 5
        for n in ROW_COUNTS[rs]:
            if n == N_TABLE:
                _, _, sums = tb.oracle(**kw)
            else:
                part, _, sums = tb.oracle(n, **kw)
                assert not bad_rows(part, whole[:n * rs], n, rs)   # the independence the test rests on
            check_against_oracle(tb, tb.decode(n, **kw), (whole[:n * rs], 5, sums), n, f"rs={rs} {kind} nr={n}")


def decode_all(tb, iterations, convergence_eps, s_clip, s_damping):
    """fwav_decode_all (one C-ABI call that resolves every exact check itself) → (recon, iterations, deltas)."""
    from fwav._lib import call, size_call
    dev = torch.device("cuda", 0)
    nr, rs = tb.nr, tb.rs
    a = torch.empty(nr * rs, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    deltas = torch.zeros(max(iterations, 1), dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    wsn = size_call("fwav_decode_all_workspace_size", nr, rs, iterations)
    ws = torch.empty(wsn, dtype=torch.uint8, device=dev)
    call("fwav_decode_all", *[t.data_ptr() for t in tb.dev[:4]], nr, rs, tb.dev[4].data_ptr(), len(tb.pool), iterations,
         float(convergence_eps), float(abs(np.float32(s_clip))), float(s_damping), a.data_ptr(), b.data_ptr(),
         deltas.data_ptr(), state.data_ptr(), ws.data_ptr(), wsn, torch.cuda.current_stream().cuda_stream)
    st = state.cpu().numpy()
    ran = int(st[1])
    return (b if st[2] == 1 else a).cpu().numpy(), ran, deltas.cpu().numpy()[:ran].tolist()


@pytest.mark.parametrize("kind", ["tiny", "flush", "huge"])
def test_delta_regimes(kind):
    """Δ sums in float32's denormal (× 1e-20, × 1e-30) and overflow (× 1e19) range: dec_decide's second arm sends the
    iteration to the exact check, and k_decode_exact has to reproduce the reference's sdot with denormal products,
    denormal sqrt and quotient, and overflow to inf.  Every parameter set whose oracle run passes through such an
    iteration (asserted on the oracle's own float64 sums), through fwav_decode_all and through
    fwav.hipctypes.decompress: the reference's Δ exactly at every checked iteration, the oracle's iteration count
    and reconstruction.  In at least one case per kind the reference stops early on the exact check's word alone:
    after 1 iteration × 1e-20 and × 1e-30, after 2 × 1e19 with damping (Δ₁ = inf, Δ₂ = x / inf = 0; on the 67-row
    table — on 300 rows ‖next − rec‖ overflows as well and Δ₂ is NaN).  rs 8: the register-resident kernel, rs 40: the
    streaming path."""
    from fwav import hipctypes
    early = 0
    for rs, nr in ((8, 67), (8, 300), (40, 67), (40, 300)):
        tb = Table(rs, nr, kind)
        cases = 0
        for pi, p in enumerate(DE.PARAMS):
            kw = DE.kw(p)
            want = tb.oracle(**kw)
            _, it, sums = want
            chk, ext = checked_iterations(sums, nr * rs, kw["convergence_eps"])
            if not ext:
                continue
            cases += 1
            early += (it == 1 and p[0] > 1) if kind != "huge" else (it == 2 and p[0] > 2 and p[3] > 0)
            for name, got in (("fwav_decode_all", decode_all(tb, *p)),
                              ("hipctypes.decompress", hipctypes.decompress(*tb.host(), **kw))):
                where = f"{name} rs={rs} nr={nr} {kind} set {pi + 1}"
                check_against_oracle(tb, got, want, nr, where)
                for t in chk:
                    assert same(got[2][t], sums[t][1]), (where, t, got[2][t], sums[t])
        assert cases >= 6, (rs, nr, cases)
    assert early >= 1


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_edges(world):
    """The sharded C-ABI sequence on the edge table (three blocks, the last one a single range): bit-identical to the
    single-device decode and to the oracle, the Δ at checked iterations included."""
    from test_gpu_decode import _shard_decode
    nr = N_TABLE + 4096
    for kind in ("finite", "tiny", "huge"):
        tb = Table(8, nr, kind)
        bounds = dist.decode_bounds(nr, world)
        assert bounds[0][0] == 0 and bounds[-1][1] == nr
        for p in (DE.PARAMS[0], DE.PARAMS[3]):
            kw = DE.kw(p)
            want = tb.oracle(**kw)
            one = tb.decode(**kw)
            where = f"world={world} {kind} {p}"
            check_against_oracle(tb, one, want, nr, where)
            outs = _shard_decode(*tb.host()[:5], 8, bounds, p[0], p[1], p[3])
            rec = np.concatenate([r.cpu().numpy() for r, _, _ in outs])
            assert not bad_rows(rec, one[0], nr, 8), where
            chk, _ = checked_iterations(want[2], nr * 8, p[1])
            for _, ran, dl in outs:
                assert ran == one[1] and len(dl) == len(one[2]) and all(same(a, b) for a, b in zip(dl, one[2])), where
                assert all(same(dl[t], want[2][t][1]) for t in chk), where


@pytest.mark.parametrize("rs", [3, 130])
def test_api_and_limits(rs):
    """fwav.api.decompress_audio on the finite and non-finite tables: matches as a list of tuples (as_match_arrays),
    sym as Python bools, an original_len that cuts the last range — equal to the oracle.  range_size 1025 (above
    kMaxPairwise) raises and returns nothing."""
    from fwav import api
    from fwav._lib import FwavError
    nr = 67
    for kind in ("finite", "nonfinite"):
        tb = Table(rs, nr, kind)
        matches = [(int(i), float(s), float(o), bool(y), 0.0) for i, s, o, y in zip(tb.idx, tb.s, tb.o, tb.sym)]
        cut = nr * rs - (rs // 2 + 1)
        for p in (DE.PARAMS[0], DE.PARAMS[4], DE.PARAMS[6]):
            kw = DE.kw(p)
            out, info = api.decompress_audio(matches, tb.pool, nr, rs, original_len=cut, return_info=True, **kw)
            with np.errstate(all="ignore"):
                ref, it, sums = O.decode(tb.idx, tb.s, tb.o, tb.sym != 0, tb.pool, nr, rs, original_len=cut,
                                         deltas="sums", **kw)
            assert out.shape == (cut,) and DE.same_bits_or_nan(out, ref), (rs, kind, p)
            assert info["iterations"] == it
            assert all(DE.same_delta(a, q[0], q[1]) for a, q in zip(info["deltas"], sums)) and len(sums) == it
    tb = Table(4, 67, "finite")
    pool = td(np.zeros(DE.N_POOL * 1025, np.float32))
    got = None
    with pytest.raises(FwavError):
        got = engine.decompress_device(*tb.dev[:4], pool, 67, 1025)
    assert got is None
