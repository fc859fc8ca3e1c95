// ftl_raymask.hpp -- the candidate rays of one sensor as bits of a pass-wide mask (phase 3 of ftl_rays_kernel, mask form).
//
// The ray sensors scanned in one pass share an index space: ray i of a sensor whose first ray has index rbase is ray rbase + i of the
// pass (FtlRaySensor::rbase).  When the pass has at most 64 rays, everything one segment can be hit by fits in one 64-bit word, bit g
// for ray g.  Host and device compile the same function; tests/test_raymask_host.py checks it against the plain enumeration.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTL_RAYMASK_FN __host__ __device__ __forceinline__
#else
#define FTL_RAYMASK_FN inline
#endif

// Bits rbase + ((i0 + t) mod N) for t = 0 .. cnt-1: the cnt consecutive rays from i0, wrapped modulo N, of a sensor of N rays.
// 1 <= N <= 64, rbase >= 0, rbase + N <= 64, 0 <= cnt <= N, -N <= i0 < 2 N (one conditional add or subtract wraps it, as the list
// form wraps every ray index).  A run of cnt ones is rotated left by the wrapped start inside an N-bit field; the part pushed out at
// the top comes back in at the bottom.  Fields of up to 32 rays are worked in 32-bit words (a 64-bit shift by a per-lane amount is
// several instructions on gfx950); no shift amount reaches the width of its word.
FTL_RAYMASK_FN uint64_t ftl_ray_mask(int i0, int cnt, int N, int rbase) {
    const int s = i0 < 0 ? i0 + N : (i0 >= N ? i0 - N : i0);       // [0, N)
    if (N <= 32) {
        const uint32_t ones = cnt >= 32 ? 0xffffffffu : (1u << cnt) - 1u;
        const uint32_t field = N >= 32 ? 0xffffffffu : (1u << N) - 1u;
        const uint32_t f = ((ones << s) | ((ones >> 1) >> (N - 1 - s))) & field;      // (>> 1 first: N - s is N when s == 0)
        return (uint64_t)f << rbase;
    }
    const uint64_t ones = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull;
    const uint64_t field = N >= 64 ? ~0ull : (1ull << N) - 1ull;
    const uint64_t f = ((ones << s) | ((ones >> 1) >> (N - 1 - s))) & field;
    return f << rbase;
}
