"""The recorded side of the engineered hysteresis cases (test helper, shared by tests/test_long_scans_cpu.py and
tests/test_gpu_long_scans.py): tests/golden/long_scans.npz read once, a case's recorded reference mask, and the
preconditions every test asserts on a case before it compares anything."""
import functools
import json
import os

import numpy as np

import front_edges as FE
from oracle import fractal_oracle as O

F32 = np.float32


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "long_scans.npz"))
    return {k: fx[k] for k in ("nf", "first", "offsets", "changes")}, json.loads(str(fx["params"]))


def recorded_mask(case):
    """The reference's per-frame mask of `case`, u8[nf]."""
    fx, meta = fixture()
    k = meta["names"].index(case.name)
    assert fx["nf"][k] == case.nf and meta["frames"][k] == case.frame and meta["windows"][k] == case.window
    return FE.mask_from_runs(int(fx["first"][k]), fx["changes"][fx["offsets"][k]:fx["offsets"][k + 1]], case.nf)


def preconditions(case, sig):
    """What `case` is there for, asserted on the oracle's smoothed energies of its signal (no device involved):
    scan_profile reaches every count of case.need; each A_KEEP run is undecided (all of it without smoothing, all
    but the frames the 5-tap window blurs at its ends with it) and its undecided frames come out with the state the
    case claims; every other run holds a decision.  → the profile."""
    hi, lo = F32(FE.VOICED_THR), F32(FE.VOICED_THR * 0.5)
    e = O.frame_energies(sig, case.frame)
    if case.window > 1:
        e = O.smooth5(e, case.window)[:case.nf]   # fewer frames than taps: np.convolve returns one value per tap
    assert len(e) == case.nf
    prof, _ = FE.scan_profile(e, hi, lo)
    for k, v in case.need.items():
        assert prof[k] >= v, (case.name, k, prof[k], v)
    dec = (e > hi) | (e < lo)
    state = FE.sequential_mask(e, hi, lo) if case.nf <= 8192 else O.hysteresis(e, hi, lo)
    at = 0
    for lev, n in case.runs:
        if lev != FE.A_KEEP:
            assert dec[at:at + n].any(), (case.name, "a run that decides nothing", at, n)
        at += n
    for a, b, st in FE.scan_claims(case):
        und = ~dec[a:b]
        assert und.sum() >= (b - a) - (0 if case.window == 1 else 5), (case.name, a, b, int(und.sum()))
        assert (state[a:b][und] == st).all(), (case.name, a, b, st)
    return prof
