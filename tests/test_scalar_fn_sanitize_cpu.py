"""Host-code sanitizers for the scalar function extension's front end: the
expression compiler (csrc/compile.cpp) built with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone program (tests/native/
scalar_fn_driver.cpp) that compiles function expressions, provokes each
compile error, calls dfmi_scalar_function_meta with short and NULL outputs
and names that are not NUL-terminated, and compiles random function
expressions. Device code is not sanitized."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_scalar_function_front_end_under_asan_ubsan(tmp_path):
    out = str(tmp_path / "scalar_fn_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", out,
           os.path.join(HERE, "native", "scalar_fn_driver.cpp"),
           os.path.join(ROOT, "datafusion_amd", "csrc", "compile.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "scalar function driver: clean" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
