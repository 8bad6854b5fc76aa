"""Generate tests/golden/long_scans.npz from the REFERENCE itself (the development container only; see make_golden.py
for how the reference is imported — the inert ``librosa`` stub).

Run:  python tests/golden/make_long_scans.py

The inputs are the engineered hysteresis signals of tests/front_edges.py (scan_cases() and PRODUCT_CASE): runs of
frames between the two thresholds that span whole waves and blocks of k_frame_state and the waves and loop trips of
k_voiced_carry (fwav_signal.hip).  Every mask is what the reference's voiced_detection (fractal.py:880-909) returns,
at thresholds 1e-4 / 5e-5, stored as run lengths.  The file holds only data:
  params     JSON: names (the cases in order), frames, windows, inputs (SHA-256 of every signal: they are rebuilt
             from their seeds, not stored)
  nf         i64[cases]      frames of each case
  first      u8[cases]       the mask's value at frame 0
  offsets    i64[cases + 1]  case k's changes are changes[offsets[k]:offsets[k + 1]]
  changes    i64[…]          the frames at which the per-frame mask changes value

The archive is written with fixed time stamps, so that a second run reproduces the committed file byte for byte."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_front_edges import frame_mask, write_npz  # noqa: E402
from make_golden import _import_reference  # noqa: E402

import front_edges as FE  # noqa: E402


def main():
    F = _import_reference()
    cases = FE.scan_cases() + [FE.PRODUCT_CASE]
    assert len({c.name for c in cases}) == len(cases)
    digests, nf, first, offsets, changes = {}, [], [], [0], []
    for c in cases:
        sig = c.signal()
        digests[c.name] = FE.digest(sig)
        vm = frame_mask(F, sig, c.frame, c.window)
        assert len(vm) == c.nf
        f, ch = FE.mask_runs(vm)
        assert np.array_equal(FE.mask_from_runs(f, ch, c.nf), vm)
        nf.append(c.nf)
        first.append(f)
        changes.append(ch)
        offsets.append(offsets[-1] + len(ch))
        print(f"{c.name}: {c.nf} frames, {int(vm.sum())} voiced, {len(ch)} changes", flush=True)
    out = dict(nf=np.array(nf, np.int64), first=np.array(first, np.uint8), offsets=np.array(offsets, np.int64),
               changes=np.concatenate(changes).astype(np.int64))
    out["params"] = np.array(json.dumps(dict(
        names=[c.name for c in cases], frames=[c.frame for c in cases], windows=[c.window for c in cases],
        thresholds=[FE.VOICED_THR, FE.VOICED_THR * 0.5], inputs=digests), sort_keys=True))
    path = os.path.join(HERE, "long_scans.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
