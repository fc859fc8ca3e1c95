// ftl_crmath.hpp -- atan, sin and cos of a double, correctly rounded: evaluated in double-double (about 104 bits) and rounded once.
// The scenario generator on the GPU calls them (DevicePolicy of ftl_scenario_core.hpp) where the host's (HostPolicy) calls glibc's atan / sin / cos:
// glibc's results are within a fraction of an ulp of the exact value and equal the correctly rounded ones on every input the generator
// produced for the seeds tested (not on every double: on random doubles about once in 1,000-2,000 calls they differ), while the device
// math library's differ often enough to change the start direction of 2-12 % of the worlds.  A few calls per scenario, on one lane: speed does not matter here.
// Double-double arithmetic after Dekker / Knuth (two_sum, two_prod with an exact fma); every operation below is exact or rounded to
// nearest in IEEE double, so the functions give the same bits on the host and on the device (-ffp-contract=off; fma is explicit).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FTL_CR_FN __host__ __device__ inline
#else
#define FTL_CR_FN inline
#endif

namespace ftl_cr {

struct dd { double hi, lo; };

FTL_CR_FN dd quick_two_sum(double a, double b) { const double s = a + b; return dd{s, b - (s - a)}; }
FTL_CR_FN dd two_sum(double a, double b) {
    const double s = a + b, v = s - a;
    return dd{s, (a - (s - v)) + (b - v)};
}
FTL_CR_FN dd two_prod(double a, double b) { const double p = a * b; return dd{p, fma(a, b, -p)}; }
FTL_CR_FN dd add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return quick_two_sum(s.hi, s.lo);
}
FTL_CR_FN dd neg(dd a) { return dd{-a.hi, -a.lo}; }
FTL_CR_FN dd sub(dd a, dd b) { return add(a, neg(b)); }
FTL_CR_FN dd mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return quick_two_sum(p.hi, p.lo);
}
FTL_CR_FN dd mul_d(dd a, double b) {
    dd p = two_prod(a.hi, b);
    p.lo += a.lo * b;
    return quick_two_sum(p.hi, p.lo);
}
FTL_CR_FN dd div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    dd r = sub(a, mul_d(b, q1));
    const double q2 = r.hi / b.hi;
    r = sub(r, mul_d(b, q2));
    const double q3 = r.hi / b.hi;
    return add(quick_two_sum(q1, q2), dd{q3, 0.0});
}
FTL_CR_FN dd sqrt_dd(dd a) {                      // a > 0
    const double q = sqrt(a.hi);
    const dd r = sub(a, two_prod(q, q));
    return quick_two_sum(q, r.hi / (2.0 * q));
}

// pi / 2 as a triple double (for the reduction of sin / cos) and as a double-double
#define FTL_CR_PIO2_1 1.5707963267948966192e+00   // 0x3FF921FB54442D18
#define FTL_CR_PIO2_2 6.1232339957367660359e-17   // 0x3C91A62633145C07
#define FTL_CR_PIO2_3 -1.4973849048591698329e-33  // 0xB91F1976B7ED8FBC

// atan(t) for 0 < t <= 1 in double-double: four halvings atan(t) = 2 atan(t / (1 + sqrt(1 + t^2))) bring t below tan(pi / 64),
// then the alternating series to below 2^-110 relative
FTL_CR_FN dd atan_dd_01(dd t) {
    const dd one{1.0, 0.0};
    for (int i = 0; i < 4; i++) t = div(t, add(one, sqrt_dd(add(one, mul(t, t)))));
    const dd t2 = mul(t, t);
    dd term = t, sum = t;
    for (int n = 1; n < 24; n++) {
        term = mul(term, t2);
        const dd q = div(term, dd{(double)(2 * n + 1), 0.0});
        sum = (n & 1) ? sub(sum, q) : add(sum, q);
        if (fabs(q.hi) < 1e-40) break;
    }
    return mul_d(sum, 16.0);
}

FTL_CR_FN double atan(double x) {
    if (x != x) return x;
    const double ax = fabs(x);
    if (ax < 1e-30) return x;                                  // atan(x) rounds to x
    dd r;
    if (ax > 1e30) r = dd{FTL_CR_PIO2_1, FTL_CR_PIO2_2};     // pi/2 - 1/x rounds to pi/2's double
    else if (ax <= 1.0) r = atan_dd_01(dd{ax, 0.0});
    else r = sub(dd{FTL_CR_PIO2_1, FTL_CR_PIO2_2}, atan_dd_01(div(dd{1.0, 0.0}, dd{ax, 0.0})));
    const double v = r.hi + r.lo;
    return x < 0 ? -v : v;
}

// sin and cos of r, |r| <= pi/4 + a little, in double-double (Taylor to below 2^-110)
FTL_CR_FN void sincos_dd(dd r, dd& s, dd& c) {
    const dd r2 = mul(r, r);
    dd term = r; s = r;
    for (int n = 1; n < 20; n++) {                           // r^(2n+1) / (2n+1)!
        term = div(mul(term, r2), dd{(double)((2 * n) * (2 * n + 1)), 0.0});
        s = (n & 1) ? sub(s, term) : add(s, term);
        if (fabs(term.hi) < 1e-40) break;
    }
    term = dd{1.0, 0.0}; c = term;
    for (int n = 1; n < 20; n++) {                           // r^(2n) / (2n)!
        term = div(mul(term, r2), dd{(double)((2 * n - 1) * (2 * n)), 0.0});
        c = (n & 1) ? sub(c, term) : add(c, term);
        if (fabs(term.hi) < 1e-40) break;
    }
}

// x - k pi/2 for |x| < 2^20 (k exact in a double, k * pio2_1 and k * pio2_2 exact as double-doubles)
FTL_CR_FN void sincos(double x, double& so, double& co) {
    if (!(fabs(x) < 1048576.0)) { so = ::sin(x); co = ::cos(x); return; }     // (never: the generator's angles lie in [0, 2 pi))
    const double k = nearbyint(x / FTL_CR_PIO2_1);
    dd r = sub(dd{x, 0.0}, two_prod(k, FTL_CR_PIO2_1));
    r = sub(r, two_prod(k, FTL_CR_PIO2_2));
    r = sub(r, dd{k * FTL_CR_PIO2_3, 0.0});
    dd s, c;
    sincos_dd(r, s, c);
    const double sv = s.hi + s.lo, cv = c.hi + c.lo;
    const int q = ((int)k) & 3;
    if (q == 0) { so = sv; co = cv; }
    else if (q == 1) { so = cv; co = -sv; }
    else if (q == 2) { so = -sv; co = -cv; }
    else { so = -cv; co = sv; }
}
FTL_CR_FN double sin(double x) { double s, c; sincos(x, s, c); return s; }
FTL_CR_FN double cos(double x) { double s, c; sincos(x, s, c); return c; }

}  // namespace ftl_cr
