"""The workspace arena of the match() schedule (roma_amd/csrc/arena.h) is host-only C++: tests/arena_check.cpp exercises a
fit, an aliased overflow and an over-capacity request as a stand-alone program, compiled here with the host compiler."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cxx():
    for cxx in (os.environ.get("CXX"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++")):
        if cxx and (os.path.exists(cxx) or shutil.which(cxx)):
            return cxx
    return None


def test_arena_fit_alias_and_over_capacity(tmp_path):
    cxx = _host_cxx()
    assert cxx, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "arena_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "roma_amd", "csrc"),
                         os.path.join(ROOT, "tests", "arena_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert out.returncode == 0 and out.stdout.strip() == "arena ok", out.stdout + out.stderr
