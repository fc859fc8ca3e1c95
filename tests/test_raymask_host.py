"""csrc/ftl_raymask.hpp: the candidate rays of one sensor as bits of a pass-wide 64-bit mask (the mask form of the ray kernel's phase 3).
A stand-alone host program compiled against the header checks ftl_ray_mask(i0, cnt, N, rbase) against the plain enumeration
{rbase + ((i0 + t) mod N) : t < cnt}, exhaustively: N = 1..64, i0 in [-N, 2N), cnt in [0, N], every rbase with rbase + N <= 64
(4.5 million masks).  No GPU, no Python extension: the program can be built with host sanitizers as it stands."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include "ftl_raymask.hpp"

int main() {
    unsigned long long checked = 0;
    for (int N = 1; N <= 64; N++)
        for (int i0 = -N; i0 < 2 * N; i0++)
            for (int cnt = 0; cnt <= N; cnt++) {
                uint64_t want0 = 0;                      // the enumeration at rbase = 0
                for (int t = 0; t < cnt; t++) want0 |= 1ull << (((i0 + t) % N + N) % N);
                for (int rbase = 0; rbase + N <= 64; rbase++) {
                    const uint64_t want = want0 << rbase, got = ftl_ray_mask(i0, cnt, N, rbase);
                    if (got != want) {
                        printf("MISMATCH N=%d i0=%d cnt=%d rbase=%d got=%016llx want=%016llx\n", N, i0, cnt, rbase,
                               (unsigned long long)got, (unsigned long long)want);
                        return 1;
                    }
                    checked++;
                }
            }
    printf("checked %llu\n", checked);
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler found")


def test_mask_equals_the_enumeration_exhaustively(tmp_path):
    src = tmp_path / "raymask_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "raymask_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # sum over N of 3N (N + 1) (65 - N) masks
    assert out.stdout.strip() == "checked %d" % sum(3 * n * (n + 1) * (65 - n) for n in range(1, 65)), out.stdout
