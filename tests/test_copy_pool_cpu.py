"""CPU: the host entry point's copy pool (csrc/ffddp_copy_pool.hpp) through
its stand-alone stress program (csrc/copy_pool_stress.cpp), built here with
plain g++ (no HIP, no GPU, no sanitizer): every destination byte right after
back-to-back 4 MiB runs on 16 threads, uneven multi-job runs with a zero-fill
among them, the caller-only path below 4 MiB, a one-thread pool, empty job
lists and pools destroyed with and without a run()."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "franka-force-feedback-mpc_amd" / "csrc"


def test_header_is_host_only():
    text = (CSRC / "ffddp_copy_pool.hpp").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_copy_pool_stress(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the copy pool's stress program cannot be built")
    exe = tmp_path / "copy_pool_stress"
    subprocess.run([cxx, "-O2", "-std=c++17", "-pthread", "-o", str(exe), str(CSRC / "copy_pool_stress.cpp")],
                   check=True, timeout=120)
    # 2000 back-to-back rounds: about a second; the 20 000-round default is the make targets'
    r = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2000 back-to-back rounds, ok" in r.stdout
