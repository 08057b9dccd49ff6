"""The byte work of correcting bases inside the mates' overlap (csrc/ffq_correctwalk.h: a chunk of sixteen overlap positions
from four loads bounded by their lines, mate 2 reversed and complemented in registers, the masks of the bytes to rewrite) on a
CPU: tests/correct_walk_host.cpp drives the functions the kernel calls against a loop over bytes -- every n1, n2 up to 40 with
every valid o, seeded cases up to 512 -- plain and under AddressSanitizer + UBSan, on buffers allocated exactly.  A stand-alone
program, never loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("san", ("", "address,undefined"))
def test_correct_walk_on_the_host(tmp_path, san):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    if san:
        # (looked for BEFORE anything is compiled: a build line that breaks is a failure, not a skip)
        res = subprocess.run([CLANG, "-print-resource-dir"], capture_output=True, text=True).stdout.strip()
        if not any(f.startswith("libclang_rt.asan") and f.endswith(".a")
                   for _d, _s, fs in os.walk(os.path.join(res, "lib")) for f in fs):
            pytest.skip("this clang++ has no AddressSanitizer runtime for the host")
    exe = tmp_path / "correct_walk_host"
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "fastq-and-furious_amd", "csrc"),
           os.path.join(ROOT, "tests", "correct_walk_host.cpp"), "-o", str(exe)]
    if san:
        cmd[1:1] = ["-fsanitize=" + san, "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert " 0 failures" in p.stdout
