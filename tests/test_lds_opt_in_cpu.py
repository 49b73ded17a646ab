"""egotap_amd/csrc/lds_opt_in.h, the bookkeeping behind ego_allow_dynamic_lds: tests/lds_opt_in_main.cpp (8 threads x 16 kernels x 4 devices,
every order, several rounds) asserts one "make the HIP call" per (kernel, device), one more for a larger size, none for a smaller one.
Built and run twice as a plain child process: as it is, and with -fsanitize=thread (the table is shared by every launcher)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "lds_opt_in_main.cpp")
INC = os.path.join(REPO, "egotap_amd", "csrc")


def _cxx():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    raise RuntimeError("no host C++ compiler found")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread"]], ids=["plain", "tsan"])
def test_lds_opt_in_threads(tmp_path, flags):
    exe = str(tmp_path / "lds_opt_in")
    cc = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-pthread", *flags, "-I" + INC, SRC, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr, run.stdout + run.stderr
    assert "64 pairs, 8 threads: ok" in run.stdout
