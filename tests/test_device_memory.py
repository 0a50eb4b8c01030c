"""Device memory has one owner per object (csrc/lb_arena.h): no other source of the library allocates or frees, and the
arena with its regrow frame behaves as stated - checked by a host-only program, tools/arena_check.cpp."""
import os
import re
import shutil
import subprocess

import pytest

from lagrangebench_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree)\w*\s*\(")
# (file, call) -> why that call stays outside the arena
ALLOWED = {("lb_msplit.hip", "hipMalloc"): "ms_dbg_buf: the process-lifetime stamp buffer of -DLB_MS_STAMPS debug builds, never freed"}


def test_only_the_arena_allocates_or_frees():
    assert "lb_arena.h" in build.HEADERS
    found = {}
    for name in build.SOURCES + build.HEADERS:
        with open(os.path.join(build.CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                for m in RAW.finditer(line):
                    found.setdefault((os.path.basename(name), m.group(0).rstrip("( \t")), []).append(no)
    outside = {k: v for k, v in found.items() if k[0] != "lb_arena.h"}
    stray = {k: v for k, v in outside.items() if k not in ALLOWED or len(v) != 1}
    assert not stray, f"raw allocation calls outside lb_arena.h: {stray}"
    assert set(outside) == set(ALLOWED), "an allow-list entry no longer matches anything: remove it"
    assert any(k[0] == "lb_arena.h" for k in found)


def test_arena_check_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "arena_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "arena_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "arena_check: ok" in r.stdout, r.stdout + r.stderr
