"""Host-code sanitizers for the context shift: csrc/tests/context_shift_selftest.cpp drives Scheduler::shift
(csrc/runtime/runtime_core.h) randomly next to the prefix cache, compiled as a stand-alone program with
AddressSanitizer + UndefinedBehaviorSanitizer and, separately, with the libstdc++ debug-mode checks, and run on the
CPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "csrc" / "tests" / "context_shift_selftest.cpp"


@pytest.mark.parametrize("flags", [
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
    ["-D_GLIBCXX_ASSERTIONS", "-D_GLIBCXX_DEBUG"],
], ids=["asan_ubsan", "glibcxx_debug"])
def test_context_shift_under_sanitizers(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, str(SRC), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "context shift selftest ok" in r.stdout
