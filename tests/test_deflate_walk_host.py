"""The parts of the BGZF deflate that have no device in them (csrc/ffq_deflatewalk.h, the functions k_deflate_members calls) on a
CPU: tests/deflate_walk_host.cpp emulates a workgroup lane by lane, builds whole gzip members from those functions and has
zlib judge them -- inflate (raw, -15) gives the block back, the CRC is crc32()'s, every code's Kraft sum is exactly 1 (a
single symbol: two codes of length 1; no match: one distance code of length 0; one distance symbol: one of length 1), the
length limits 15 and 7 are reached on Fibonacci counts, the CRC combine agrees with zlib's for 1, 2 and 255 segments and a
short last one -- plain and under AddressSanitizer + UBSan.  A stand-alone program, never loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("san", ("", "address,undefined"))
def test_deflate_walk_on_the_host(tmp_path, san):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    if san:
        # (looked for BEFORE anything is compiled: a build line that breaks is a failure, not a skip)
        res = subprocess.run([CLANG, "-print-resource-dir"], capture_output=True, text=True).stdout.strip()
        if not any(f.startswith("libclang_rt.asan") and f.endswith(".a")
                   for _d, _s, fs in os.walk(os.path.join(res, "lib")) for f in fs):
            pytest.skip("this clang++ has no AddressSanitizer runtime for the host")
    exe = tmp_path / "deflate_walk_host"
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "fastq-and-furious_amd", "csrc"),
           os.path.join(ROOT, "tests", "deflate_walk_host.cpp"), "-lz", "-o", str(exe)]
    if san:
        cmd[1:1] = ["-fsanitize=" + san, "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert " 0 failures" in p.stdout
