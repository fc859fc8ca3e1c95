// ftl_rnn_math.hpp -- the transcendentals of the recurrent policy (include/ftl.h, the ftl_rnn_act block): exp32, sig32 and tanh32 as fixed
// sequences of float32 operations, the same on the host and on the device.  Every line is one float32 operation with one IEEE rounding;
// the unit that includes this is built with -ffp-contract=off, so no line fuses with its neighbour, and without any fast-math or
// denormal-flushing option, so the divisions are the correctly rounded ones (__fdiv_rn on the device says so whatever the build's default)
// and subnormals are kept.  tests/rnn_numpy.py is the numpy twin; tests/test_rnn_host.py compiles this header for the host and compares
// the two bit for bit.
//
// Accuracy against the float64 value: exp32 within 0.92 ulp on [-86, 0]; sig32 within 8.91e-8 and tanh32 within 8.93e-8 absolute.  Near 0
// tanh32 computes (1 - e) / (1 + e) with e close to 1: the RELATIVE error of the result is large there by cancellation (tanh32(1e-8) is
// 0, not 1e-8).  That is accepted: the cell adds these values to numbers of order 1.
#ifndef FTL_RNN_MATH_HPP
#define FTL_RNN_MATH_HPP
#include <math.h>

#if defined(__HIPCC__)
#define FTL_RNN_HD __host__ __device__
#else
#define FTL_RNN_HD
#endif

namespace ftlrnnmath {

FTL_RNN_HD inline float div32(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// e^a for a <= 0 (a below -86, and a NaN, are read as -86: sig32 and tanh32 return a NaN argument before they get here)
FTL_RNN_HD inline float exp32(float a) {
    a = fmaxf(a, -86.0f);
    const float s = a * 0x1.715476p+0f;                        // a * log2(e)
    const float n = rintf(s);                                  // ties to even
    float r = fmaf(n, -0x1.62e400p-1f, a);                     // a - n * ln2, in two parts (bits 0x3f317200, 0x35bfbe8e)
    r = fmaf(n, -0x1.7f7d1cp-20f, r);
    float p = 0x1.a01a02p-13f;                                 // 1/5040
    p = fmaf(p, r, 0x1.6c16c2p-10f);                           // 1/720
    p = fmaf(p, r, 0x1.111112p-7f);                            // 1/120
    p = fmaf(p, r, 0x1.555556p-5f);                            // 1/24
    p = fmaf(p, r, 0x1.555556p-3f);                            // 1/6
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return ldexpf(p, (int)n);
}

FTL_RNN_HD inline float sig32(float x) {
    if (x != x) return x;
    const float e = exp32(-fabsf(x));
    const float d = 1.0f + e;
    return x >= 0.0f ? div32(1.0f, d) : div32(e, d);
}

FTL_RNN_HD inline float tanh32(float x) {
    if (x != x) return x;
    const float m = -2.0f * fabsf(x);
    const float e = exp32(m);
    const float a = 1.0f - e;
    const float b = 1.0f + e;
    return copysignf(div32(a, b), x);
}

}  // namespace ftlrnnmath
#endif
