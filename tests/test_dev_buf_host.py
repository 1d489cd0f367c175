"""csrc/dev_buf.hpp on the host: tests/dev_buf_host/main.cpp (malloc-backed raw allocation, no GPU runtime) built
with AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process.  Moves, self-moves, alloc over a
live buffer, registry entries that follow their buffers through a growing std::vector, and nothing left once
everything is destroyed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dev_buf_host", "main.cpp")
CSRC = os.path.join(ROOT, "recommendation-models_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_dev_buf_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "dev_buf_host")
    # the sanitizer runtimes linked statically (clang's default): the program needs nothing preloaded
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + ([] if clang else ["-static-libasan", "-static-libubsan"]) +
                   ["-I", CSRC, "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "dev_buf ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
