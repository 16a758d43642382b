"""The tile layout builder (csrc/tile_layout.h: the plan-time grouping of every (window, tile) task's slots by neighbour
id for csrc/kernels_tile.h) against brute force, on the CPU: tests/host/tile_layout_check.cpp is compiled as a
stand-alone program -- with the address and undefined-behaviour sanitizers where the compiler has them; the test
prints which build ran (pytest -s or the captured output of a failure) -- and run.
It replays the kernel's index arithmetic over the layout of small random graphs (several and ragged tiles, a hub
column, a hub row cut into pieces, empty rows, rectangular shapes, result buffers smaller than a task) and checks the
slot and distinct-neighbour counts per task, records of at most four slots, that the result offsets are a permutation
of the task's slots with every row piece's results one contiguous run, and that every edge id is written exactly once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "tile_layout_check.cpp")
INC = os.path.join(ROOT, "custom_op_benchmark_amd", "csrc")


def _compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_tile_layout_against_brute_force(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tile_layout_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I" + INC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:                           # a toolchain without the sanitizer runtimes: the checks still run
        print("tile_layout_check: the sanitizer build failed, running the plain build:\n" + r.stderr[-2000:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("tile_layout_check built %s" % ("with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), \
        ("sanitized build" if sanitized else "plain build") + ":\n" + run.stdout + run.stderr
