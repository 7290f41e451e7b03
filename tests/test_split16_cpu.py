"""csrc/split16.h on the host: tools/split16_check.cpp (the exact three-way bf16 split of the bf16x6 GEMM route) built without
sanitizer flags and run.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split16_check_builds_and_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "split16_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "vatl4pose-wacv2024_amd", "csrc"),
                    os.path.join(ROOT, "tools", "split16_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
