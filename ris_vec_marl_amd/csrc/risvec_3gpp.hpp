// The 3GPP TR 38.901-style channel gain of one (env, vehicle) (RIS ignored; ENV:8-25, 275-327): position -> LOS draw ->
// path loss -> log-normal shadow -> small-scale power -> float32 gain.  Shared by the stand-alone k_gain_3gpp
// (k_env.hip) and the fused 3GPP step family (k_step_3gpp.hip): one body, so the fused forms reproduce the two-launch
// form bit for bit by construction.  Contraction is pinned (fp contract(on): a * b + c inside one expression only), so
// the result cannot depend on what the calling kernel puts around it.  10^x is exp10(x), not pow(10, x): the general
// float64 pow (a log and an exp in extended precision) was the largest single cost of the gain.
//
// The pieces are split at what depends on the position only (geo_3gpp, large_3gpp) and what is drawn afresh every call
// (draws_3gpp, gain_3gpp_draw): the T-step kernel hoists the first half out of its step loop.
#pragma once

#include "risvec_launch.hpp"

namespace risvec {

// ENV:29-42
__device__ constexpr double kBsX = 0.0, kBsY = 0.0, kBsZ = 25.0;
__device__ constexpr double kVehZ = 1.5;

// u ~ U[0,1) (LOS decision, ENV:299), z ~ N(0,1) (shadow, ENV:10), sm = small-scale power (ENV:13-25)
struct Draws3gpp {
    double u, z, sm;
};

// Philox draws of (global env genv, vehicle v) at `counter`: sites kSite3gpp and, for Rice, kSite3gpp + 0x100
__device__ __forceinline__ Draws3gpp draws_3gpp(float rician_k_db, uint32_t genv, uint32_t v, uint32_t counter,
                                                uint64_t seed) {
#pragma clang fp contract(on)
    Draws3gpp r;
    const uint4 x = philox4x32_10(genv, v, counter, kSite3gpp, seed);
    r.u = u01(x.x);                                                         // ENV:299
    const float2 n = normal2(x.y, x.z);
    r.z = n.x;                                                              // ENV:10
    if (rician_k_db <= 1e-6f) {
        r.sm = -log(((double)(x.w >> 8) + 1.0) * 0x1p-24);                 // Exp(1), ENV:17
    } else {                                                                // ENV:19-25
        const uint4 x2 = philox4x32_10(genv, v, counter, kSite3gpp + 0x100u, seed);
        const float2 n2 = normal2(x2.x, x2.y);
        const double K = exp10((double)rician_k_db / 10.0);
        const double s = sqrt(K / (K + 1.0)), sg = 1.0 / sqrt(2.0 * (K + 1.0));
        const double hr = s + sg * n2.x, hi = sg * n2.y;
        r.sm = hr * hr + hi * hi;
    }
    return r;
}

// what depends on the position only
struct Geo3gpp {
    double d2d;          // horizontal distance to the BS
    double ld, lf;       // log10(max(d3d, 1)), log10(fc / GHz)
};

__device__ __forceinline__ Geo3gpp geo_3gpp(const RisVecParams& P, double x, double y) {
#pragma clang fp contract(on)
    Geo3gpp g;
    const double dx = fabs(x - kBsX), dy = fabs(y - kBsY);
    const double dz = fabs(kBsZ - kVehZ);
    g.d2d = hypot(dx, dy);
    const double d3d = sqrt(g.d2d * g.d2d + dz * dz);
    g.ld = log10(fmax(d3d, 1.0));
    g.lf = log10((double)P.fc_ghz);
    return g;
}

// LOS probability: the draw u is LOS below it (ENV:298-299)
__device__ __forceinline__ double p_los_3gpp(const Geo3gpp& g) { return 0.7 * exp(-g.d2d / 200.0); }

// linear large-scale gain 10^(-PL/10) of the model; RISVEC_CH_OTHER: 0 dB (ENV:315-317)
__device__ __forceinline__ double large_3gpp(const RisVecParams& P, int model, bool los, const Geo3gpp& g) {
#pragma clang fp contract(on)
    const double ld = g.ld, lf = g.lf;
    double pl_db = 0.0;
    if (model == RISVEC_CH_3GPP_UMI)
        pl_db = los ? 32.4 + 21.0 * lf + 20.0 * ld : 36.7 + 22.7 * lf + 26.0 * ld;       // ENV:281,285
    else if (model == RISVEC_CH_3GPP_UMA)
        pl_db = los ? 28.0 + 22.0 * lf + 20.0 * ld
                    : 13.54 + 39.08 * ld + 20.0 * lf - 0.6 * (double)P.veh_ant_gain;     // ENV:289,293
    return exp10(-pl_db / 10.0);
}

// large x shadow x small-scale power (ENV:10-11, 327)
__device__ __forceinline__ float gain_3gpp_draw(const RisVecParams& P, double large, bool los, const Draws3gpp& r) {
#pragma clang fp contract(on)
    const double sd = los ? (double)P.shadow_std_los : (double)P.shadow_std_nlos;
    const double shadow = exp10((r.z * sd) / 10.0);
    return (float)(large * shadow * r.sm);
}

// the whole chain for one (env, vehicle) at position (x, y) with draws r
__device__ __forceinline__ float gain_3gpp(const RisVecParams& P, int model, double x, double y, const Draws3gpp& r) {
    const Geo3gpp g = geo_3gpp(P, x, y);
    const bool los = r.u < p_los_3gpp(g);
    return gain_3gpp_draw(P, large_3gpp(P, model, los, g), los, r);
}

}  // namespace risvec
