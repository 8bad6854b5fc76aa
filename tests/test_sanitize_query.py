"""Host-side AddressSanitizer + UndefinedBehaviorSanitizer run of the entry points that take a query table of their
own (compress_audio(query="range")): tests/sanitize/query_check.cpp, a stand-alone program, linked against the same
host-instrumented objects as tests/test_sanitize.py's plan_check (every .hip source with -Xarch_host -fsanitize=...,
device code compiled normally and never launched).  Argument checks, the seed window's clamped centre and the work
plan with more query rows than domains.  CPU only; nothing is preloaded."""
import hashlib
import os
import shutil
import subprocess

import pytest

import test_sanitize as S

DRIVER = os.path.join(S.ROOT, "tests", "sanitize", "query_check.cpp")


def _build() -> str:
    S._build()  # the sanitized objects of every .hip source, rebuilt when the sources changed
    from fwav import _digest
    key = hashlib.sha256((_digest.source_digest() + open(DRIVER).read() + " ".join(S.FLAGS)).encode()).hexdigest()
    exe = os.path.join(S.OUT, "query_check")
    stamp = exe + ".key"
    if os.path.exists(exe) and os.path.exists(stamp) and open(stamp).read() == key:
        return exe
    obj = os.path.join(S.OUT, "query_check.o")
    subprocess.check_call(["hipcc", *S.FLAGS, "-x", "hip", "-c", DRIVER, "-o", obj])
    objs = [os.path.join(S.OUT, f[:-4] + ".o") for f in sorted(os.listdir(S.CSRC)) if f.endswith(".hip")]
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", *S.SAN, *objs, obj, "-o", exe])
    with open(stamp, "w") as f:
        f.write(key)
    return exe


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_query_table_entry_points_under_asan_ubsan():
    exe = _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "0 failures" in r.stdout and "plans with more queries than domains" in r.stdout
