"""csrc/ftl_trktrim.hpp: the trim test of the v2 tracker (path_length > corridor_length, sensors.py:288-297) decided from the exact float64
sum W of the window's float32 segment lengths.  Python builds the cases with numpy and writes them to a file -- the reference answer is
np.sum(d.astype(np.float32)) > L, numpy's own pairwise sum; a stand-alone host program compiled against the header reads them, forms W
in float64 and reports the decided answers that are wrong and the undecided ones.  No GPU, no Python extension: the program has its own
main and can be built with host sanitizers as it stands.

Cases: n = 1..520 terms; spacings U(0.5, 30), constant, U(1e-4, 1), |N(7.5, 3)|; for each, L random, L equal to the float32 sum and
its two float32 neighbours.  No decided answer may be wrong.  On a stream like config B's (L = 250, segments U(5, 10), one append per
call, popped while the float32 sum exceeds L) at most 1 % of the tests may come back undecided."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "continiousenvironment_follower_leader_amd", "csrc")

# case file: int32 count, then per case: int32 n, int32 want (0 keep / 1 pop), float64 L, n float32 terms
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ftl_trktrim.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    long long wrong = 0, undecided = 0;
    std::vector<float> d;
    for (int k = 0; k < count; k++) {
        int n = 0, want = 0; double L = 0.0;
        if (fread(&n, 4, 1, f) != 1 || fread(&want, 4, 1, f) != 1 || fread(&L, 8, 1, f) != 1 || n < 0 || n > 4096) return 2;
        d.resize((size_t)n);
        if (n > 0 && fread(d.data(), 4, (size_t)n, f) != (size_t)n) return 2;
        double W = 0.0;
        for (int i = 0; i < n; i++) W += (double)d[(size_t)i];      // exact for these terms (checked in Python)
        const int dec = ftl_trk_trim(W, L, 0.0);
        if (dec == FTL_TRIM_UNDECIDED) undecided++;
        else if ((dec == FTL_TRIM_POP) != (want != 0)) {
            if (wrong < 10) printf("WRONG case %d n=%d W=%.17g L=%.17g decided %d want %d\n", k, n, W, L, dec, want);
            wrong++;
        }
    }
    fclose(f);
    printf("cases %d wrong %lld undecided %lld\n", count, wrong, undecided);
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("trktrim")
    src = d / "trktrim_check.cpp"
    src.write_text(PROGRAM)
    exe = d / "trktrim_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    return str(exe)


def _run(program, path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for d, L, want in cases:
            f.write(struct.pack("<iid", len(d), int(want), float(L)))
            f.write(np.asarray(d, np.float32).tobytes())
    out = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().split("\n")[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(cases), out.stdout
    return int(last[3]), int(last[5]), out.stdout


def _exact_terms(d):
    """the terms as the kernel keeps them: float32, none below 2^-20 unless zero, and their in-order float64 sum exact"""
    d = np.asarray(d, np.float64).astype(np.float32)
    d[(d != 0) & (d < np.float32(2.0 ** -20))] = np.float32(2.0 ** -20)
    w = 0.0
    for v in d:
        w += float(v)
    assert w == math.fsum(float(v) for v in d)
    return d


def test_no_wrong_decision_on_random_windows_and_at_the_knife_edge(program, tmp_path):
    rng = np.random.default_rng(20240607)
    cases = []
    for n in range(1, 521):
        for kind in range(4):
            if kind == 0:
                d = rng.uniform(0.5, 30.0, n)
            elif kind == 1:
                d = np.full(n, rng.uniform(0.5, 30.0))
            elif kind == 2:
                d = rng.uniform(1e-4, 1.0, n)
            else:
                d = np.abs(rng.normal(7.5, 3.0, n))
            d = _exact_terms(d)
            p = np.sum(d.astype(np.float32))               # numpy's float32 pairwise sum: what the reference compares
            assert p.dtype == np.float32
            ls = [float(rng.uniform(0.0, 2.0 * float(p))), float(p),
                  float(np.nextafter(p, np.float32(np.inf))), float(np.nextafter(p, np.float32(-np.inf)))]
            # thresholds around the EXACT sum as well: where the float32 sum and the exact one may fall on different sides
            s = float(np.sum(d.astype(np.float64)))
            ls += [s, float(np.nextafter(np.float32(s), np.float32(np.inf))), float(np.nextafter(np.float32(s), np.float32(-np.inf)))]
            for L in ls:
                cases.append((d, L, bool(float(p) > L)))
    wrong, undecided, text = _run(program, tmp_path / "cases.bin", cases)
    print("cases %d undecided %d" % (len(cases), undecided))
    assert wrong == 0, text
    # L equal to the float32 sum is inside the band by the band's derivation; of the seven thresholds of a window only the random
    # one is far from both sums
    assert undecided >= 520 * 4, text
    assert undecided <= 6 * 520 * 4 + 50, text


def test_a_stream_like_config_b_is_hardly_ever_undecided(program, tmp_path):
    rng = np.random.default_rng(7)
    L = 250.0
    win = []
    cases = []
    for _ in range(40000):
        win.append(np.float32(rng.uniform(5.0, 10.0)))
        while True:                                        # one trim test per loop trip, as the kernel makes them
            d = np.asarray(win, np.float32)
            pop = bool(float(np.sum(d)) > L)
            cases.append((d, L, pop))
            if not pop:
                break
            win.pop(0)
    wrong, undecided, text = _run(program, tmp_path / "stream.bin", cases)
    share = undecided / len(cases)
    print("stream: tests %d undecided %d (%.4f %%)" % (len(cases), undecided, 100.0 * share))
    assert wrong == 0, text
    assert share <= 0.01, text
