"""What a lane does when a UMI is taken off a read and put into its name (csrc/ffq_umiwalk.h, the functions the kernels of
csrc/ffq_umi.h call) on a CPU: tests/umi_walk_host.cpp drives them against loops over bytes -- the first blank and the newline
look over sixteen bytes, the cut, a carrier's positions, and a tagged row assembled chunk by chunk from the spans of its pieces at
every shift of the output address -- plain and under AddressSanitizer + UBSan.  A stand-alone program, never loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("san", ("", "address,undefined"))
def test_umi_walk_on_the_host(tmp_path, san):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    if san:
        # (looked for BEFORE anything is compiled: a build line that breaks is a failure, not a skip)
        res = subprocess.run([CLANG, "-print-resource-dir"], capture_output=True, text=True).stdout.strip()
        if not any(f.startswith("libclang_rt.asan") and f.endswith(".a")
                   for _d, _s, fs in os.walk(os.path.join(res, "lib")) for f in fs):
            pytest.skip("this clang++ has no AddressSanitizer runtime for the host")
    exe = tmp_path / "umi_walk_host"
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "fastq-and-furious_amd", "csrc"),
           os.path.join(ROOT, "tests", "umi_walk_host.cpp"), "-o", str(exe)]
    if san:
        cmd[1:1] = ["-fsanitize=" + san, "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert " 0 failures" in p.stdout
