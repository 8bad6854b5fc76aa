"""Generate tests/golden/decode_edges.npz from the REFERENCE itself (the development container only; see make_golden.py
for how the reference is imported — the inert ``librosa`` stub — and how ``run_decode`` reads the iteration count and
the Δ values off its log).

Run:  python tests/golden/make_decode_edges.py

For every entry of tests/decode_edges.fixture_entries() — range sizes on every dispatch path of fwav_decode, the five
value kinds (finite, non-finite, ×1e-20, ×1e-30, ×1e19), the parameter sets of decode_edges.PARAMS — the edge table of
tests/decode_edges.build goes through the reference's own ``decompress_audio`` (fractal.py:1378-1473).  The file holds
only data: a JSON string (entries, parameter sets, the SHA-256 of every built input — the inputs themselves are rebuilt
by the tests) and per entry
  it_<tag>    iterations run
  dl_<tag>    f64[it]: the Δ values as the log prints them ({delta:.6e})
  dig_<tag>   u8[nr, 8]: per range, the first 8 bytes of SHA-256 of its reconstruction with every NaN made the one
              quiet NaN (decode_edges.row_digests) — all 480 reconstructions themselves would be 8 MB
  rec_<tag>   f32[nr·rs]: the reconstruction itself, for the default parameters at range sizes ≤ 40."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _import_reference, run_decode  # noqa: E402

import decode_edges as DE  # noqa: E402

REC_MAX_RS = 40


def tag(rs, kind, pi):
    return f"rs{rs}_{kind}_p{pi}"


def main():
    F = _import_reference()
    nr = DE.FIXTURE_NR
    entries = DE.fixture_entries()
    out, digests, tables = {}, {}, {}
    for rs, kind, pi in entries:
        if (rs, kind) not in tables:
            idx, s, o, sym, pool, _ = DE.build(rs, nr, kind)
            tables[rs, kind] = (idx, s, o, sym, pool)
            digests[f"rs{rs}_{kind}"] = DE.input_digest(idx, s, o, sym, pool)
        idx, s, o, sym, pool = tables[rs, kind]
        matches = [(int(idx[i]), float(s[i]), float(o[i]), int(sym[i]), 0.0) for i in range(nr)]
        with np.errstate(all="ignore"):
            rec, it, dl = run_decode(F, matches, pool, nr, rs, None, **DE.kw(DE.PARAMS[pi]))
        t = tag(rs, kind, pi)
        out[f"it_{t}"] = np.int32(it)
        out[f"dl_{t}"] = dl
        out[f"dig_{t}"] = DE.row_digests(rec, nr, rs)
        if pi == 0 and rs <= REC_MAX_RS:
            out[f"rec_{t}"] = rec
        print(t, it, dl[:3], flush=True)
    out["params"] = np.array(json.dumps(dict(
        nr=nr, rs=list(DE.FIXTURE_RS), kinds=list(DE.KINDS), params=[list(p) for p in DE.PARAMS],
        entries=[[rs, kind, pi] for rs, kind, pi in entries], inputs=digests)))
    np.savez_compressed(os.path.join(HERE, "decode_edges.npz"), **out)


if __name__ == "__main__":
    main()
