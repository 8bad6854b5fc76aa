"""The sequential part of the hysteresis on the device (fwav_signal.hip: k_voiced_decide → k_voiced_carry →
k_frame_state) on the engineered signals of front_edges.scan_cases(): undecided runs that span whole waves and blocks
of k_frame_state's max-scan, the 64-block waves of k_voiced_carry and the trips of its loop (1024 blocks each) —
tests/test_gpu_front_edges.py's signals keep inside all of them.

Every case first asserts in numpy what it is there for (long_scans.preconditions: on the oracle's smoothed energies,
before the device is touched), then calls fwav_voiced_ranges through test_gpu_front_edges.check_voiced: the mask
equals the reference's recorded one (tests/golden/long_scans.npz) and O.voiced_detection, the ranges equal
O.form_ranges bit for bit, and the call with mask_out = NULL gives the same ranges.  No case is left out."""
import numpy as np
import pytest

import front_edges as FE
import long_scans as LS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import engine  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402
from test_gpu_front_edges import check_voiced, td  # noqa: E402

F32 = np.float32
LISTS = FE.scan_lists()
SMALL = [k for k in LISTS if not k.startswith("trip")]
TRIPS = [c for k in LISTS if k.startswith("trip") for c in LISTS[k]]
HI, LO = F32(FE.VOICED_THR), F32(FE.VOICED_THR * 0.5)


def run_case(case):
    sig = case.signal()
    prof = LS.preconditions(case, sig)
    check_voiced(sig, case.frame, case.window, HI, LO, LS.recorded_mask(case), case.name, null_mask=True)
    return prof


@pytest.mark.parametrize("name", SMALL)
def test_runs_across_threads_waves_blocks_and_the_carrys_waves(name):
    """The in-block lists (a decision at frame p around 4, 256 and 1024, then 1 … 3·1024 + 5 undecided frames, both
    polarities, and the leading run): k_frame_state's wlast = −1 behind a decisive wave and blast = −1 with the carry
    from further back.  The wave lists (65, 66 and 130 blocks, frames 8, 38 and 64): the only decision in block 0,
    63 or 64, or a voiced one in block 0 and an unvoiced one in block 64 — k_voiced_carry's second and third wave
    take their prefix from wsum."""
    total = {}
    for case in LISTS[name]:
        for k, v in run_case(case).items():
            total[k] = total.get(k, 0) + v
    print(name, len(LISTS[name]), "cases:", total)
    if name.startswith("inblock"):
        assert total["carried_waves"] >= 100 and total["far_blocks"] >= 18
    else:
        assert total["wave_crossings"] >= 100


@pytest.mark.parametrize("case", TRIPS, ids=repr)
def test_runs_across_the_carrys_trips(case):
    """1025, 1026 and 2049 blocks: `running` leaves k_voiced_carry's first trip — the only decision in block 0, an
    unvoiced one in the last block of trip 1 or the first of trip 2, the only (voiced) one in the last block of
    trip 1, and a trip without any decision that hands trip 1's voiced state on to trip 3."""
    prof = run_case(case)
    assert prof["trip_crossings"] >= 1
    if "skip" in case.name or case.name.endswith("2049_only0"):
        assert prof["trip_skips"] >= 1


def test_product_call_carries_the_state_over_three_blocks():
    """engine.compress_device on a loud start, more than three blocks of undecided frames and silence: res.ranges are
    the oracle's (the undecided blocks voiced, the silence zero), and the same signal through fwav_voiced_ranges."""
    case = FE.PRODUCT_CASE
    sig = case.signal()
    prof = LS.preconditions(case, sig)
    assert prof["undecided_blocks"] >= 3 and prof["far_blocks"] >= 2
    check_voiced(sig, case.frame, case.window, HI, LO, LS.recorded_mask(case), case.name, null_mask=True)
    res = engine.compress_device(td(sig), FE.PRODUCT_TILE, 4, energy_thresh=FE.VOICED_THR, keep_intermediates=True,
                                 tie_order="index")
    torch.cuda.synchronize()
    assert res.range_size * 2 == case.frame and not res.empty
    vm = O.voiced_detection(sig, case.frame, FE.VOICED_THR)
    want, _ = O.form_ranges(sig, vm, res.range_size)
    got = res.ranges.cpu().numpy().reshape(-1, res.range_size)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    a, b, st = FE.scan_claims(case)[0]
    assert st == 1 and vm[a * case.frame:(b - 3) * case.frame].all() and not vm[(b + 3) * case.frame:].any()
