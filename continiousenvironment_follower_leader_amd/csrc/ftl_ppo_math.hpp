// ftl_ppo_math.hpp -- the row arithmetic of the PPO loss head (include/ftl.h, the ftl_ppo_head block) and its per-set scalars, the same
// on the host and on the device.  Every line is one operation with one IEEE rounding -- float32 in the row, float64 in the set scalars --;
// the unit that includes this is built with -ffp-contract=off, so no line fuses with its neighbour.  div32 and exp32 are those of
// ftl_rnn_math.hpp.  tests/ppo_numpy.py is the numpy twin; tests/test_ppo_host.py compiles this header for the host and compares the two
// bit for bit.
#ifndef FTL_PPO_MATH_HPP
#define FTL_PPO_MATH_HPP
#include <math.h>

#include "ftl_rnn_math.hpp"

namespace ftlppomath {

// what a set's rows share: sigma_new, sigma_old and c = log_std_new - log_std_old per component, the advantage's mean and inverse
// deviation rounded to float32, 1 / count, and the call's scalars
struct Set {
    float sigma_new[2], sigma_old[2], shift[2];
    float mean32, inv32, invc;
    float clip_lo, clip_hi, vf_coef;
    int normalize, has_value;
};

// what a row yields: its gradients and the float32 values that the reductions widen to float64
struct Row {
    float dhead[2], dvalue;
    float ratio, pl, vl, nd, k[2];      // r; -min(s1, s2); 0.5 (v - ret)^2; -d; the row's share of d loss / d log_std_new
    int clipped;                        // r < clip_lo || r > clip_hi
};

template <int A>
FTL_RNN_HD inline void row(const Set& s, const float* head_new, const float* head_old, const float* noise, float adv, float ret, float v, Row& o) {
    using ftlrnnmath::div32;
    using ftlrnnmath::exp32;
    float u[2], p[2], l[2];
    for (int j = 0; j < A; j++) {
        const float e = head_old[j] - head_new[j];
        const float t = fmaf(s.sigma_old[j], noise[j], e);
        u[j] = div32(t, s.sigma_new[j]);
        p[j] = u[j] * u[j];
        const float q = noise[j] * noise[j];
        const float w = q - p[j];
        l[j] = fmaf(0.5f, w, -s.shift[j]);
    }
    const float d = A == 1 ? l[0] : l[0] + l[1];
    float r;
    if (d != d) r = d;
    else if (d <= 0.0f) r = exp32(d);
    else r = div32(1.0f, exp32(-d));
    float a = adv;
    if (s.normalize) {
        const float am = adv - s.mean32;
        a = am * s.inv32;
    }
    const float s1 = r * a;
    const float rc = fminf(fmaxf(r, s.clip_lo), s.clip_hi);
    const float s2 = rc * a;
    const bool active = !(s2 < s1);
    float g = 0.0f;
    if (active) {
        const float t = s1 * s.invc;
        g = -t;
    }
    for (int j = 0; j < A; j++) {
        const float us = div32(u[j], s.sigma_new[j]);
        o.dhead[j] = g * us;
        const float pm = p[j] - 1.0f;
        o.k[j] = g * pm;
    }
    if (A == 1) { o.dhead[1] = 0.0f; o.k[1] = 0.0f; }
    o.ratio = r;
    o.pl = -(active ? s1 : s2);
    o.nd = -d;
    o.clipped = (r < s.clip_lo || r > s.clip_hi) ? 1 : 0;
    o.dvalue = 0.0f;
    o.vl = 0.0f;
    if (s.has_value) {
        const float hv = v - ret;
        const float vh = s.vf_coef * hv;
        o.dvalue = vh * s.invc;
        const float hh = hv * hv;
        o.vl = 0.5f * hh;
    }
}

FTL_RNN_HD inline double sqrt64(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// the per-set scalars from the count and the float64 totals of adv and adv * adv
struct Moments { double mean, std; float mean32, inv32, invc; };

FTL_RNN_HD inline Moments moments(double cnt, double S1, double S2) {
    Moments m;
    m.mean = cnt > 0.0 ? S1 / cnt : 0.0;
    double var = 0.0;
    if (cnt >= 2.0) {
        const double t = S1 * m.mean;
        const double w = S2 - t;
        const double c1 = cnt - 1.0;
        const double q = w / c1;
        var = q < 0.0 ? 0.0 : q;                               // max(q, 0) that keeps a NaN
    }
    m.std = sqrt64(var);
    const double se = m.std + 1e-8;
    const double inv = 1.0 / se;
    m.mean32 = (float)m.mean;
    m.inv32 = (float)inv;
    m.invc = 0.0f;
    if (cnt > 0.0) {
        const double ic = 1.0 / cnt;
        m.invc = (float)ic;
    }
    return m;
}

}  // namespace ftlppomath
#endif
