"""fwav_affine called directly, against the reference's own outputs (tests/golden/affine_edges.npz) and against
O.affine (pinned to that fixture by tests/test_oracle_golden.py::test_affine_edges_pinned), over its three dispatch
paths — k_affine_batch (rs 4/8/16, K ≤ 64), k_affine<RS> (rs 4/8/16, K > 64), k_affine_any (any other rs) — on the
edge table of tests/affine_edges.py: all-(−1) rows, −1 tails, only the last slot valid, constant tiles and ranges,
mirror pairs in both slot orders, palindromes, one domain twice, s clipped at ±16 / 0.5, overflow, inf, NaN (the first
NaN wins), tiny values, then random rows; K on both sides of 64 and row counts that do not fill the kernels' 16-range
workgroups.

Bar: every output bit-equal, except that a NaN matches any NaN (sign and payload differ between x86 numpy and the
device and are not compared)."""
import os

import numpy as np
import pytest

import affine_edges as AE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav._lib import call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

NAMES = ("idx", "s", "o", "sym", "err")


def dev():
    return torch.device("cuda", 0)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Solver:
    """The table on the device once; solve(a, b, s_clip) runs fwav_affine on rows [a, b) alone."""

    def __init__(self, ranges, cand, pool):
        self.rs, self.K, self.nd = ranges.shape[1], cand.shape[1], len(pool)
        self.ranges, self.cand, self.pool = td(ranges.reshape(-1)), td(cand.reshape(-1)), td(pool.reshape(-1))

    def solve(self, a, b, s_clip=16.0):
        n = b - a
        out = [torch.empty(n, dtype=dt, device=dev()) for dt in
               (torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32)]
        call("fwav_affine", self.ranges[a * self.rs:].data_ptr(), n, self.rs, self.cand[a * self.K:].data_ptr(),
             self.K, self.pool.data_ptr(), self.nd, float(s_clip), *[t.data_ptr() for t in out],
             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]


def test_device_equals_the_reference_fixture():
    """The device against the reference's own _flush_gpu_batch outputs, every recorded shape and s_clip."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "affine_edges.npz"))
    for rs, K in AE.FIXTURE_SHAPES:
        tag = f"rs{rs}_k{K}"
        sv = Solver(fx[f"ranges_{tag}"], fx[f"cand_{tag}"], fx[f"pool_{tag}"])
        for ci, sc in enumerate(fx["s_clips"].tolist()):
            got = sv.solve(0, AE.N_ROWS, sc)
            for nm, a in zip(NAMES, got):
                want = fx[f"{nm}_{tag}_c{ci}"]
                bad = [i for i in range(AE.N_ROWS) if not AE.same_bits_or_nan(a[i:i + 1], want[i:i + 1])]
                assert not bad, f"{tag} s_clip={sc} {nm}: rows {bad}: device {a[bad]} reference {want[bad]}"


@pytest.mark.parametrize("rs", AE.RS_ALL)
def test_affine_sweep_against_oracle(rs):
    """rs × K ∈ {1, 2, 63, 64, 65, 129} × rows ∈ {1, 15, 16, 17, 67}: every slice of the table solved on its own equals
    the same rows of O.affine on the whole table (rows are independent); s_clip 0.5 and −16 on the 67-row call."""
    for K in AE.K_ALL:
        ranges, cand, pool, names = AE.build(rs, K)
        with np.errstate(all="ignore"):
            want = {sc: O.affine(ranges, cand, pool, s_clip=sc) for sc in (16.0, 0.5, -16.0)}
        sv = Solver(ranges, cand, pool)
        label = names + ["random"] * (AE.N_ROWS - len(names))
        for n in AE.ROWS_ALL:
            for a, b in AE.slices(n):
                if n == 1 and a >= len(names) + 3:  # single-row calls: every edge row and three random ones
                    continue
                for sc in ((16.0, 0.5, -16.0) if n == AE.N_ROWS else (16.0,)):
                    got = sv.solve(a, b, sc)
                    for nm, g, w in zip(NAMES, got, want[sc]):
                        w = np.asarray(w)[a:b]
                        bad = [i for i in range(b - a) if not AE.same_bits_or_nan(g[i:i + 1], w[i:i + 1])]
                        assert not bad, (f"rs={rs} K={K} rows [{a}, {b}) s_clip={sc} {nm}: "
                                         f"{[(a + i, label[a + i], g[i], w[i]) for i in bad[:5]]}")
