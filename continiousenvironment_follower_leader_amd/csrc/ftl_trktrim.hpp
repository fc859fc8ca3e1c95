// ftl_trktrim.hpp -- the trim test of LeaderPositionsTracker_v2.scan (sensors.py:288-297) decided from a running corridor length.
//
// The reference pops the oldest history point while  path_length > corridor_length,  where path_length is numpy's float32 pairwise sum p of
// the n float32 segment lengths of the window.  The frame kernel keeps W, the EXACT sum S of the same n values, in float64 (ftl_frames_group.hpp,
// g_sensors: every non-zero segment is >= 2^-20 and W < 2^10, so all terms are multiples of 2^-43 and every W += d, W -= d is exact).  p differs
// from S only by float32 rounding; outside a band around the threshold, S decides the test the reference makes on p.
//
// The band.  All terms are non-negative, so every partial sum of the float32 evaluation is a sum of terms, and each float32 addition
// multiplies the partial sums that enter it by (1 + e), |e| <= u = 2^-24.  A term that passes through k additions on its way to the result
// therefore arrives scaled by a factor within [(1 - u)^k, (1 + u)^k], and  |p - S| <= ((1 + u)^K - 1) S  with K the largest k of any term.
// numpy's pairwise sum (umath pairwise_sum, the order g_pw128 / g_pw reproduce):
//   n < 8             one accumulator, in order: K = n - 1 <= 6;
//   8 <= n <= 128     eight interleaved accumulators, each the in-order sum of floor(n / 8) <= 16 terms (<= 15 additions), three combining
//                     additions ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 <= 7 tail terms added in order: K <= 15 + 3 + 7 = 25;
//   n > 128           two halves (the first a multiple of 8), recursively, one addition per level: a leaf holds at most 128 terms, and
//                     n <= 1024 makes at most three levels: K <= 25 + 3 = 28  (the kernel's windows stop at 512 terms: two levels).
// (1 + u)^28 - 1 < 28.01 u.  The band used is 32 u S = 2^-19 S: the slack of almost 4 u S also covers the float64 roundings of the test
// itself (W * 2^-19 is exact; W - L rounds by at most 2^-53 max(W, L), eight orders below u S wherever the band matters) .
// FTL_DEBUG_TRK_BAND widens the band by a fixed number of pixels (`extra`), for the tests of the undecided path.
//
// Host and device compile the same function; tests/test_trktrim_host.py checks it against np.sum of the float32 terms.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTL_TRKTRIM_FN __host__ __device__ __forceinline__
#else
#define FTL_TRKTRIM_FN inline
#endif

enum { FTL_TRIM_KEEP = 0, FTL_TRIM_POP = 1, FTL_TRIM_UNDECIDED = 2 };

// half-width of the band around `corridor_length` inside which W does not decide: 32 * 2^-24 * W + extra
FTL_TRKTRIM_FN double ftl_trk_band(double W, double extra) { return W * 1.9073486328125e-06 + extra; }   // 2^-19

// The reference's  path_length > corridor_length  from the exact length W of the window (W >= 0, W < 2^10, at most 1024 terms):
// FTL_TRIM_POP / FTL_TRIM_KEEP when the float32 pairwise sum cannot lie on the other side of the threshold, FTL_TRIM_UNDECIDED exactly
// when |W - corridor_length| is inside the band -- the caller then evaluates the pairwise sum itself.
FTL_TRKTRIM_FN int ftl_trk_trim(double W, double corridor_length, double extra) {
    const double band = ftl_trk_band(W, extra), diff = W - corridor_length;
    if (diff > band) return FTL_TRIM_POP;
    if (-diff > band) return FTL_TRIM_KEEP;
    return FTL_TRIM_UNDECIDED;
}
