"""CPU pins of the engineered hysteresis signals (no GPU): tests/golden/long_scans.npz holds the reference's own
voiced masks (tests/golden/make_long_scans.py), as run lengths, of the signals of front_edges.scan_cases() — runs of
frames between the two thresholds that span whole waves and blocks of k_frame_state and the waves and loop trips of
k_voiced_carry (fwav_signal.hip).

Here: the builders still make the recorded inputs (digests); O.voiced_detection reproduces every recorded mask, which
makes it the reference of tests/test_gpu_long_scans.py; and every case is what it claims to be — the counts it is
there for (front_edges.scan_profile on the oracle's smoothed energies) and the state its undecided runs come out
with (long_scans.preconditions, the same function the GPU tests call before they touch the device)."""
import numpy as np
import pytest

import front_edges as FE
import long_scans as LS
from oracle import fractal_oracle as O

LISTS = FE.scan_lists()
SMALL = [k for k in LISTS if not k.startswith("trip")]
TRIPS = [c for k in LISTS if k.startswith("trip") for c in LISTS[k]]


def test_fixture_lists_the_cases_the_builders_make():
    fx, meta = LS.fixture()
    cases = FE.scan_cases() + [FE.PRODUCT_CASE]
    assert meta["names"] == [c.name for c in cases] and len(set(meta["names"])) == len(cases)
    assert meta["frames"] == [c.frame for c in cases] and meta["windows"] == [c.window for c in cases]
    assert fx["nf"].tolist() == [c.nf for c in cases]
    assert meta["thresholds"] == [FE.VOICED_THR, FE.VOICED_THR * 0.5]
    # every size and position the lists are made of
    names = set(meta["names"])
    for w in FE.SCAN_WINDOWS:
        for pol in ("voiced", "unvoiced"):
            assert all(f"inblock_w{w}_{pol}_p{p}_L{L}" in names for p in FE.IN_BLOCK_P for L in FE.IN_BLOCK_L)
        assert f"inblock_w{w}_leading" in names
        for nb in FE.WAVE_BLOCKS:
            assert all(f"wave_f8_w{w}_{nb}_{p}" in names for p in ("only0", "only63", "only64", "v0_u64"))
        for nb in FE.TRIP_BLOCKS:
            assert all(f"trip_w{w}_{nb}_{p}" in names for p in ("only0", "v0_u1023", "v0_u1024", "only1023"))
        assert f"trip_w{w}_2049_u0_v700_skip" in names
    for f in (38, 64):
        assert all(f"wave_f{f}_w5_{nb}_v0_u64" in names for nb in FE.WAVE_BLOCKS)
    assert max(c.nf * c.frame for c in cases) == 2049 * 1024 * 8


def check_case(case):
    """Digest, preconditions, and the oracle's mask against the reference's recorded one → the case's profile."""
    sig = case.signal()
    assert FE.digest(sig) == LS.fixture()[1]["inputs"][case.name], case.name
    prof = LS.preconditions(case, sig)
    vm = O.voiced_detection(sig, case.frame, FE.VOICED_THR, smooth_window=case.window)
    assert len(vm) == len(sig)
    assert np.array_equal(vm[::case.frame], LS.recorded_mask(case)), case.name
    return prof


@pytest.mark.parametrize("name", SMALL)
def test_oracle_mask_is_the_reference_in_block_and_across_the_carrys_waves(name):
    """The in-block and wave lists: digests, each case's own preconditions, the oracle's mask; and over a whole list
    the counts the list is there for — an in-block list holds hundreds of whole undecided waves behind a decisive
    one and thousands of such 4-frame groups, a wave list over a hundred carries into another 64-block wave."""
    total = {}
    for case in LISTS[name]:
        for k, v in check_case(case).items():
            total[k] = total.get(k, 0) + v
    print(name, len(LISTS[name]), "cases:", total)
    assert total["trip_crossings"] == 0     # these lists stay inside the carry's first trip
    if name.startswith("inblock"):
        assert total["carried_threads"] >= 1000 and total["carried_waves"] >= 100 and total["far_blocks"] >= 18
        assert total["wave_crossings"] == 0
    else:
        assert total["wave_crossings"] >= 100 and total["undecided_blocks"] >= 1000


@pytest.mark.parametrize("case", TRIPS, ids=repr)
def test_oracle_mask_is_the_reference_across_the_carrys_trips(case):
    """At least 1025 blocks with at most two decisions (and, smoothed, the cut-short windows of the first and last
    frame): more than a thousand blocks without one, and a block of trip 2 whose state comes from trip 1."""
    prof = check_case(case)
    assert prof["trip_crossings"] >= 1 and prof["undecided_blocks"] >= 1025 - 4


def test_product_case():
    prof = check_case(FE.PRODUCT_CASE)
    assert prof["undecided_blocks"] >= 3 and prof["far_blocks"] >= 2
    # compress_device's geometry at this tile is the case's: frame = 2 · range size, and the ranges fit the pool
    from fwav import geometry
    rs, step = geometry(FE.PRODUCT_TILE)
    n = len(FE.PRODUCT_CASE.signal())
    assert 2 * rs == FE.PRODUCT_CASE.frame and -(-n // rs) <= (n - FE.PRODUCT_TILE) // step + 1


def test_profile_counts_by_hand():
    """scan_profile on energies written by hand: decisions at frames 0 (voiced) and 1024·65 + 7 (unvoiced) of 131
    blocks, and one of 2049 blocks with a decision at frame 3 alone."""
    e = np.full(131 * 1024, 7e-5, np.float32)
    e[0], e[65 * 1024 + 7] = 1.0, 0.0
    prof, src = FE.scan_profile(e)
    assert prof == dict(decisive=2, carried_threads=63 + 62, carried_waves=3 + 3, undecided_blocks=129,
                        leading_blocks=0, far_blocks=64 + 64, wave_crossings=2 + 3, trip_crossings=0, trip_skips=0)
    assert src.tolist() == [-1] + [0] * 65 + [65] * 65
    e = np.full(2049 * 1024, 7e-5, np.float32)
    e[3] = 1.0
    prof, src = FE.scan_profile(e)
    assert (prof["leading_blocks"], prof["far_blocks"], prof["wave_crossings"]) == (1, 2047, 2048 - 63)
    assert (prof["trip_crossings"], prof["trip_skips"], prof["carried_threads"]) == (1025, 1, 63)
    first, changes = FE.mask_runs(O.hysteresis(e, 1e-4, 5e-5))
    assert (first, changes.tolist()) == (0, [3])
    assert FE.mask_from_runs(1, [2, 5], 7).tolist() == [1, 1, 0, 0, 0, 1, 1]
