"""The C-ABI library: loads on CPU, exports exactly what include/fwav.h declares, binds with the right arity,
rejects bad arguments with status codes (no GPU needed: argument checks run before any HIP call).  The debug library
(libfwav_debug.so, include/fwav_debug.h) adds the search's test knobs; the product library exports none of them."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fwav.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "fwav_debug.h")


def header_functions(path=HEADER):
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*(?:const\s+)?[\w]+\s*\*?\s*(fwav_\w+)\s*\(([^;]*?)\);", txt, flags=re.M | re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib


def test_header_symbols_exported(lib):
    decl = header_functions()
    assert len(decl) >= 15
    dll = ctypes.CDLL(lib.LIB_PATH)
    for name in decl:
        assert hasattr(dll, name), f"{name} declared in include/fwav.h but not exported"


def test_bindings_match_header(lib):
    decl = header_functions()
    assert set(decl) == set(lib.SIGNATURES), set(decl) ^ set(lib.SIGNATURES)
    for name, n in decl.items():
        assert len(lib.SIGNATURES[name][1]) == n, name


def test_debug_library_split(lib):
    """include/fwav_debug.h declares exactly the debug bindings; libfwav_debug.so exports them and every product entry
    point, libfwav.so none of them (no process-global knob in the product library)."""
    decl = header_functions(DEBUG_HEADER)
    assert set(decl) == set(lib.DEBUG_SIGNATURES), set(decl) ^ set(lib.DEBUG_SIGNATURES)
    for name, n in decl.items():
        assert len(lib.DEBUG_SIGNATURES[name][1]) == n, name
    prod = ctypes.CDLL(lib.LIB_PATH)
    dbg = ctypes.CDLL(lib.DEBUG_LIB_PATH)
    for name in decl:
        assert hasattr(dbg, name) and not hasattr(prod, name), name
    for name in header_functions():
        assert hasattr(dbg, name), name
    assert lib.debug_lib().fwav_build_digest() == lib.product_lib().fwav_build_digest()
    # the knobs are reachable only through debug_library(), which resets them on exit
    with lib.debug_library() as d:
        assert lib.lib() is d
        lib.call("fwav_debug_topk_geometry", 0)
    assert lib.lib() is lib.product_lib()


def test_every_knob_is_guarded():
    """Every compile-time knob of the kernels (#ifndef / #ifdef FWAV_TOPK_* / FWAV_AFF_*) is named in its file's
    product-build guard (#error without -DFWAV_DEBUG_API), so no -D override can reach libfwav.so."""
    import re
    for f, pre in (("fwav_topk.hip", "FWAV_TOPK_"), ("fwav_affine.hip", "FWAV_AFF_")):
        src = open(os.path.join(ROOT, "audio-compression_amd", "csrc", f)).read()
        knobs = set(re.findall(r"#ifn?def (" + pre + r"\w+)", src))
        guard = src[src.index("#if !defined(FWAV_DEBUG_API) && ("):]
        guard = guard[:guard.index("#error")]
        named = set(re.findall(r"defined\((" + pre + r"\w+)\)", guard))
        assert knobs and knobs <= named, (f, sorted(knobs - named))
    # the search's private headers define no switch: one moved there would escape the guard above
    import glob
    heads = sorted(glob.glob(os.path.join(ROOT, "audio-compression_amd", "csrc", "fwav_topk*.h")))
    assert heads
    for h in heads:
        assert not re.findall(r"#\s*ifn?def\s+(?:FWAV_TOPK_|FWAV_FLOOR_)\w*", open(h).read()), h


@pytest.mark.parametrize("switch", ["FWAV_TOPK_ABL=1", "FWAV_TOPK_CPMIN=4", "FWAV_TOPK_W=4", "FWAV_TOPK_G=2",
                                    "FWAV_TOPK_CB=4"])
def test_product_build_refuses_experiment_switches(switch):
    """An experiment code path compiled without -DFWAV_DEBUG_API stops the build (#error): the product library can
    carry none of them (libfwav_debug.so, built with -DFWAV_DEBUG_API, is where they compile)."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "audio-compression_amd", "csrc", "fwav_topk.hip")
    cmd = ["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", f"-D{switch}", src]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "experiment switches build the debug library only" in out.stderr


def test_error_codes_without_gpu(lib):
    L = lib.lib()
    assert L.fwav_abi_version() == 5
    rc = L.fwav_affine(None, 10, 8, None, 64, None, 100, 16.0, None, None, None, None, None, None)
    assert rc == -1 and b"null" in L.fwav_last_error()
    rc = L.fwav_sim_topk(None, None, 10, None, None, 10, 0, 64, 1, None, None, None, 0, None)
    assert rc == -1
    big = ctypes.c_void_p(16)
    rc = L.fwav_sim_topk(big, None, 10, big, big, 10, 0, 64, 0, big, None, None, 0, None)
    assert rc == -1 and b"blas_threads" in L.fwav_last_error()
    rc = L.fwav_sim_topk(big, None, 10, big, big, 10, 0, L.fwav_topk_max_k() + 1, 1, big, None, None, 0, None)
    assert rc == -3 and b"K=" in L.fwav_last_error()
    rc = L.fwav_sim_topk(big, None, 10, big, big, 10, 0, 0, 1, big, None, None, 0, None)
    assert rc == -3
    # K > 64 needs the score-row workspace
    rc = L.fwav_sim_topk(big, None, 10, big, big, 10, 0, 100, 1, big, None, None, 0, None)
    assert rc == -5 and b"workspace" in L.fwav_last_error()
    rc = L.fwav_tie_check(None, 10, 8, None, 64, None, 100, None, 0, 1, None, 10, 0, None, None)
    assert rc == -1
    rc = L.fwav_score_rows(None, 100, None, 1, 0, 1, None, None)
    assert rc == -1
    # tie fix-up: null arrays with rows to apply are rejected; no rows is a no-op (no launch)
    rc = L.fwav_tie_rows_in(None, 3, None, 64, None, None, 8, None, None)
    assert rc == -1 and b"fwav_tie_rows_in" in L.fwav_last_error()
    assert L.fwav_tie_rows_in(None, 0, None, 64, None, None, 8, None, None) == 0
    rc = L.fwav_tie_rows_out(None, 3, *[None] * 10, None)
    assert rc == -1 and b"fwav_tie_rows_out" in L.fwav_last_error()
    assert L.fwav_tie_rows_out(None, 0, *[None] * 10, None) == 0
    rc = L.fwav_tie_rows_in(big, -1, big, 64, big, big, 8, big, None)
    assert rc == -2  # FWAV_ERR_SHAPE


def test_debug_search_rejects_workspace_of_another_query_count(lib):
    """Round 2's memory fault (tools/phase_ab.py): a workspace sized for 41,344 queries was handed to a search of
    20,672, whose table-pieces plan needs more key buffers.  The debug entry point now takes the workspace size and
    rejects a short one before any launch; the product always sizes for the query count it launches."""
    L = lib.debug_lib()
    nd = 1_321_977
    sizes = {q: L.fwav_sim_topk_workspace_size(q, nd, 64) for q in (20672, 41344, 65536, 82688, 131072)}
    # a workspace sized for more queries can be too small for fewer (their plan splits more blocks into pieces)
    # (the sizes also cover the centroid geometry's plans, which can make them monotonic in the query count)
    pairs = [(b, sizes[a]) for a in sizes for b in sizes if b < a and sizes[b] > sizes[a]]
    p = ctypes.c_void_p(16)
    # always: one byte short of every query count's own size, and every smaller size of another count (a larger
    # count's workspace handed to a smaller count whose plan needs more, whenever the sizes are not monotonic)
    cases = [(q, sizes[q] - 1) for q in sizes] + [(q, ws) for q in sizes for ws in sizes.values() if ws < sizes[q]]
    assert len(cases) >= 2 * len(sizes) and all(c in cases for c in pairs)
    for q, ws in cases:
        rc = L.fwav_debug_sim_topk(p, p, nd, p, p, q, 0, 64, p, p, ws, 0, None, None)
        assert rc == -5 and b"workspace" in L.fwav_last_error(), (q, ws)


def test_library_digest_matches_sources(lib):
    """The library reports the digest of the sources and flags it was built from, and it is this tree's
    (fwav._lib refuses to bind a library built from anything else)."""
    from fwav import _digest
    assert lib.lib().fwav_build_digest().decode() == _digest.source_digest()


@pytest.mark.parametrize("dbl", [0, 1])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_dct_is_scipy_bitexact(lib, n, dbl):
    """fwav_dct.h (the embedding kernel's DCT, instantiated on the host): scipy.fftpack.dct(x, norm='ortho') bit for
    bit in float32 (the tonal head, fractal.py:186) and float64 (the transient head, fractal.py:158)."""
    import scipy.fftpack
    L = lib.lib()
    T = np.float64 if dbl else np.float32
    rng = np.random.default_rng(n + 100 * dbl)
    out = np.zeros(n)
    for _ in range(4000):
        x = (rng.standard_normal(n) * rng.choice([1e-30, 1e-6, 1e-3, 1.0, 1e4])).astype(T)
        if rng.random() < 0.05:
            x[rng.integers(n)] = 0
        xin = x.astype(np.float64)
        assert L.fwav_debug_dct2(n, dbl, xin.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out.astype(T).view(np.uint8), scipy.fftpack.dct(x, norm="ortho").view(np.uint8)), x


def test_embed_tables_match_scipy_dct(lib):
    """fwav_embed_tables is a host function: its rows are the ortho DCT-II rows × linspace weights."""
    import scipy.fftpack
    L = lib.lib()
    for rs in (4, 8, 16, 13):
        tab = np.zeros(L.fwav_embed_tables_size(rs))
        assert L.fwav_embed_tables(rs, tab.ctypes.data) == 0
        eye = np.eye(rs)
        D = scipy.fftpack.dct(eye, norm="ortho", axis=0)  # D[k, n]
        w = np.linspace(1.0, 2.0, rs)
        take, tk = min(8, rs - 1), min(8, rs)
        ton = tab[:8 * rs].reshape(8, rs)
        tra = tab[8 * rs:16 * rs].reshape(8, rs)
        np.testing.assert_allclose(ton[:take], D[1:1 + take] * w[1:1 + take, None], atol=1e-14)
        np.testing.assert_allclose(tra[:tk], D[:tk] * w[None, :], atol=1e-14)
        assert np.all(ton[take:] == 0) and np.all(tra[tk:] == 0)


def test_workspace_sizes(lib):
    from fwav._lib import size_call
    assert size_call("fwav_voiced_workspace_size", 2646000, 16) > 0
    assert size_call("fwav_pool_workspace_size", 2646000, 2048, 8, 2) == ((2646000 - 2048) // 2 + 1 + 7 * 128) * 4
    assert size_call("fwav_pool_workspace_size", 1000, 2048, 8, 2) == 0
    assert size_call("fwav_sim_topk_workspace_size", 330750, 1321977, 64) >= 330750 * 64 * 8
    # K > 64: one batch of exact score rows, <= 1 GiB, at least one row
    big = size_call("fwav_sim_topk_workspace_size", 330750, 1321977, 1000)
    assert 1321977 * 4 <= big <= (1 << 30)
    assert size_call("fwav_sim_topk_workspace_size", 10, 1000, 1000) == 10 * 1000 * 4


@pytest.mark.parametrize("wide", [0, 1, 2, 3])
@pytest.mark.parametrize("n,rt,pieces", [(330750, 0, 1), (330750, 24, 4), (41344, 1 << 20, 3), (165375, 134, 4),
                                         (1000, 1 << 20, 8), (70000, 7, -1), (33, 3, 2), (256 * 5, 2, 5)])
def test_work_plan_covers_every_query(lib, n, rt, pieces, wide):
    """Host-side: the fp16 search's work plan (query blocks, INTERLEAVEd query groups, table pieces, query halves)
    runs every active query exactly once per table piece of its block and nothing past the list."""
    count = np.zeros(n, np.int32)
    items = ctypes.c_int64()
    with lib.debug_library():
        lib.call("fwav_debug_topk_plan_cover", n, rt, pieces, wide, count.ctypes.data, ctypes.addressof(items))
    qb = lib.debug_lib().fwav_debug_topk_qb(wide)  # queries per block of the geometry
    # base 8 waves × 32, wide 16 × 32, centroid 8 waves × 2 sets × 32, centroid-wide 16 × 2 × 32
    assert qb == {0: 256, 1: 512, 2: 512, 3: 1024}[wide]
    nb = -(-n // qb)
    P = 1 if pieces == 1 else (2 if pieces == -1 else pieces)
    R = 0 if P == 1 else min(nb, rt)
    assert items.value == (nb - R) + R * P
    # queries of the split blocks (the last R blocks under the interleaved mapping) are counted P times (halves: once)
    expect = np.ones(n, np.int32)
    if pieces > 1 and R:
        g = np.arange(n) // 32
        split = (g % nb) >= nb - R
        expect[split] = pieces
    assert np.array_equal(count, expect)


@pytest.mark.parametrize("nq,nd", [(330750, 1321977), (165375, 1321977), (82688, 1321977), (41344, 1321977),
                                   (32768, 1321977), (20672, 1321977), (1000, 28801), (1653750, 6613977),
                                   (2700000, 86398977)])
def test_default_plan_pieces_tile_the_table(lib, nq, nd):
    """Host-side: the default plan's table pieces (piece_chunks, uneven where a one-round plan pairs older and younger
    workgroups or a multi-round plan lightens its last piece) tile [0, ⌈nd/256⌉) without gaps or empty pieces, for
    every split block; in one rank's eighth of cfg2 a block's pieces whose items start past slot 256 (the CUs' younger
    workgroups) are the smaller ones, at cfg2 and at a quarter of it (several rounds) the last piece is."""
    nchunks = -(-nd // 256)
    for block in (0, 1, 93, 94, 160, 161, 200, 645):
        c01 = np.zeros(2 * 64, np.int32)
        n = ctypes.c_int32()
        with lib.debug_library():
            lib.call("fwav_debug_topk_piece_chunks", nq, nd, block, c01.ctypes.data, ctypes.addressof(n))
        P = n.value
        c0, c1 = c01[0:2 * P:2], c01[1:2 * P:2]
        assert 1 <= P <= 64 and c0[0] == 0 and c1[-1] == nchunks
        assert np.array_equal(c0[1:], c1[:-1]) and np.all(c1 > c0)
        size = c1 - c0
        if (nq, nd) == (41344, 1321977):  # one round of 81 blocks × 6 pieces; slots 256 + 256
            b = block % 81
            older = np.array([p * 81 + b < 256 for p in range(P)])
            assert P == 6 and older.any() and (~older).any()
            assert size[older].min() > size[~older].max(), (block, size, older)
        if (nq, nd) in ((330750, 1321977), (82688, 1321977)):  # several rounds (646 × 3, 162 × 6): the last piece lighter
            assert P == {330750: 3, 82688: 6}[nq] and size[-1] < size[:-1].min()
            assert size[:-1].max() - size[:-1].min() <= 1


_MAPS = r"""
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
{pre}
from fwav import _lib
_lib.product_lib()
hip = sorted({{l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l}})
print("HIP", "torch" in sys.modules, hip)
"""


@pytest.mark.parametrize("pre", ["", "from fwav import hipctypes\nhipctypes.hip()",
                                 "import torch\nfrom fwav import hipctypes\nhipctypes.hip()"])
def test_one_hip_runtime_per_process(lib, pre):
    """libfwav.so loaded with no torch imported yet must still leave ONE HIP runtime in the process: PyTorch-ROCm
    ships its own libamdhip64, and a library that bound the system one first left torch a second runtime that saw no
    device.  The torch-free host (fwav.hipctypes) binds the system runtime and never imports torch."""
    import subprocess
    import sys
    code = _MAPS.format(root=ROOT, pkg=os.path.join(ROOT, "audio-compression_amd"), pre=pre)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    line = [x for x in out.stdout.splitlines() if x.startswith("HIP")]
    assert out.returncode == 0 and line, out.stderr[-2000:]
    torch_loaded = line[0].split()[1] == "True"
    hip = eval(line[0].split(" ", 2)[2])
    assert len(hip) == 1, hip
    if pre and "import torch" not in pre:
        assert not torch_loaded and "/torch/" not in hip[0]
    else:  # torch first (or the product host importing it): its runtime, reused by hipctypes.hip()
        try:
            import torch  # noqa: F401
            assert torch_loaded and "/torch/" in hip[0]
        except ImportError:
            pass
