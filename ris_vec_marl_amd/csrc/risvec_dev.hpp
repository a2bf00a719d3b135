// Device-side helpers shared by the RIS-VEC kernels (gfx950 / CDNA4, wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "risvec.h"

namespace risvec {

// Kernel arguments arrive through scalar loads from a cold scalar cache (every launch starts cold): left alone, the
// compiler fetches the argument a first branch depends on, waits (~0.35 us), branches, and only then requests the
// pointers -- two or more dependent round trips in front of a kernel's first memory request.  Naming the arguments a
// kernel needs first in one `asm volatile("" :: "s"(..))` makes them one batch, one wait.  Matters for every kernel
// that lives only a few microseconds (k_step_fused_lat at BASELINE configs[1]: 0.74 -> 0.44 us before the first
// request is out; the C4 shard 8.1 -> 7.2 us per step).
#define RISVEC_ARGS_IN_ONE_TRIP(...) asm volatile("" ::__VA_ARGS__)

constexpr int kWave = 64;      // CDNA wavefront width (hard-coded on purpose)
constexpr int kBlock = 256;    // 4 waves per workgroup, one per SIMD

// Launch-time dimensions (scalars, passed by value).
struct Dims {
    int E, V, M, cbit;
    long long env_offset;
};

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  Counter = (global env id, vehicle,
// counter, site); key = 64-bit seed.  Restated bit-exactly in
// oracle/risvec_oracle.py::philox4x32.
// ---------------------------------------------------------------------------
enum Site : uint32_t {
    kSiteArrivals = 0, kSiteTurnA = 1, kSiteTurnB = 2, kSiteSpawn = 3,
    kSiteBuf0 = 4, kSite3gpp = 5, kSitePhase = 6,
    kSiteReplay = 8,   // row draw of the replay samplers (7, 9 and 10: the pairing and the policy epilogue)
    kSiteOU = 11       // OU exploration noise of the SARL rollout: c1 = pair index, .x / .y -> elements 2j / 2j + 1
};

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint64_t seed) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 64-bit product per multiplier (v_mad_u64_u32) instead of a multiply-high and a multiply-low: the same bits
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// uint32 -> float in [0,1): top 24 bits, exact in fp32.
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }

// numpy.random.randint(low, high) replacement: low + floor(x (high-low) / 2^32).
__device__ __forceinline__ int randint_u32(uint32_t x, int low, int high) {
    return low + (int)(((uint64_t)x * (uint64_t)(uint32_t)(high - low)) >> 32);
}

// Poisson(lambda) by inversion against the host-built float32 CDF table: the count
// of table entries <= u.  The loop is wave-uniform (exits when no lane advances).
// The first 8 entries are counted branch-free (a compare + add each: at the shipped rates 1 and 3 a draw above
// 7 has probability 1e-6 / 4e-3); the loop over the rest of the table runs only when some lane needs it.
__device__ __forceinline__ int poisson_from_u(float u, const float* __restrict__ cdf) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) n += u >= cdf[k] ? 1 : 0;
    if (__any(u >= cdf[7])) {
#pragma unroll 1
        for (int k = 8; k < RISVEC_POISSON_TABLE; ++k) {
            const bool ge = u >= cdf[k];
            if (!__any(ge)) break;
            n += ge ? 1 : 0;
        }
    }
    return n;
}

// standard normal pair from two uint32 (Box-Muller, fp32) -- production 3GPP path only;
// parity tests inject the reference's own draws instead.
__device__ __forceinline__ float2 normal2(uint32_t a, uint32_t b) {
    const float u1 = ((float)(a >> 8) + 1.0f) * 0x1p-24f;   // (0,1]
    const float u2 = u01(b);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    return make_float2(r * c, r * s);
}

// ---------------------------------------------------------------------------
// cross-lane: all-reduce over aligned groups of W lanes (W a power of two <= 64)
// ---------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

template <int W>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

__host__ __device__ constexpr int pow2_ceil(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// complex helpers on float2 = (re, im)
// (explicit fused forms: an `a*b - c*d` expression leaves the choice of which product is fused to the
// compiler, and it chose differently in different kernels -- results must not depend on the kernel taken)
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 acc) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.x = fmaf(-a.y, b.y, acc.x);
    acc.y = fmaf(a.x, b.y, acc.y);
    acc.y = fmaf(a.y, b.x, acc.y);
    return acc;
}

// The float32 phasor of candidate index k of a control_bit = 3 RIS: exp(j 2 pi k / 8) as the BCD sweep stores it
// (ENV:169, 213; +-1, +-0.70710677f and +0 -- every zero is +0), and 0 for k = 8, the integer 0 of ENV:211, 220.
// The one definition behind the by-index readers' table (theta_table_fill, risvec_pipe.hpp) and k_random_phase.
__device__ __forceinline__ float2 theta_candidate(int k) {
    const float r = 0.70710677f;
    float c = (k & 3) == 2 ? 0.f : ((k & 1) ? r : 1.f);
    float sn = (k & 3) == 0 ? 0.f : ((k & 1) ? r : 1.f);
    if (k >= 3 && k <= 5) c = -c;
    if (k >= 5) sn = -sn;
    return k < 8 ? make_float2(c, sn) : make_float2(0.f, 0.f);
}

// exp(j x) in float64 for |x| <= 1e5: Cody-Waite reduction by pi/2 (two-term split, exact product for |k| < 2^17) and the
// fdlibm kernel polynomials on [-pi/4, pi/4] -- error < 1e-15, i.e. the float32 image is the correctly rounded one except
// within 1e-8 ulp of a rounding boundary.  ~30 float64 instructions against the ~150 of the general sincos(), whose
// range reduction for huge arguments and special cases made k_set_phase VALU-bound (9 us for 25 MB at E = 32 768, M = 64:
// the SARL step's theta = exp(j action_phase), every step).
__device__ __forceinline__ void sincos_small(double x, double& s, double& c) {
    const double kd = rint(x * 0.63661977236758138);                        // round(x * 2/pi)
    double r = fma(-kd, 1.5707963267341256, x);                              // pi/2, high 33 bits
    r = fma(-kd, 6.0771005065061922e-11, r);                                 // pi/2, next 53 bits
    const double z = r * r;
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                                  2.75573137070700676789e-06), -1.98412698298579493134e-04),
                                 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                                  -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                 -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double sr = fma(r * z, ps, r);
    const double cr = fma(z * z, pc, fma(-0.5, z, 1.0));
    const int q = (int)kd & 3;
    const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;               // sin, cos before the signs
    s = (q & 2) ? -a : a;
    c = (q == 1 || q == 2) ? -b : b;
}

// theta = exp(j angle) as every phase setter stores it (get_next_phase, ENV:233-239): the float32 image of the float64
// phasor of the float32 angle.  One routine for k_set_phase and the SARL rollout kernel, which must agree bit for bit.
__device__ __forceinline__ float2 phasor_of_angle(float angle) {
    const double x = (double)angle;
    double s, c;
    if (fabs(x) <= 1.0e5) sincos_small(x, s, c);
    else sincos(x, &s, &c);                                                  // ENV:239
    return make_float2((float)c, (float)s);
}

// One 16-element chunk of a steering row, h_r[e,v,m0 .. m0+15] = exp(-j pi ang m), as float32 pairs: out[k] holds
// elements m0 + 2k and m0 + 2k + 1.  THE definition of the row -- k_geometry (k_env.hip) writes it to state.h_r, and the
// GEN members of the fused step (k_step_gen.hip) rebuild it from state.steer_ang / state.z_r instead of reading it, and
// must get the same bits.  One sincospi at the head of the chunk, then 15 float64 rotations by w = exp(-j pi ang) =
// (wr, wi), each element rounded once to float32.  Every product and sum is spelled out: which of the two products of
// `a * b - c * d` is fused is otherwise the compiler's choice, and two inlined copies could choose differently.  The
// association below is the one the compiler had chosen for k_geometry (read off its gfx950 code): the w-real product is
// fused and the w-imaginary product rounded first, except in the first rotation of every pair after the chunk's first,
// where it is the other way round.
//
// The routine is two: steer_head() gives the chunk's first element in float64, steer_chunk_from_head() rotates on from
// it.  The head depends on the angle alone, so it may be kept in memory (risvec_steer_heads) and the chain started from
// the stored value (the GEN members under RISVEC_STEP_STEER_HEADS_CURRENT): a float64 store and load change no bit.
constexpr int kGeoChunk = 16;

// z = exp(-j pi ang m0) = (zc, -zs)
__device__ __forceinline__ double2 steer_head(double ang, int m0) {
#pragma clang fp contract(off)
    double zs, zc;
    sincospi(__dmul_rn(ang, (double)m0), &zs, &zc);
    return make_double2(zc, -zs);
}

__device__ __forceinline__ void steer_chunk_from_head(double ar, double ai, double wr, double wi, float4 (&out)[kGeoChunk / 2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < kGeoChunk; k += 2) {
        const double br = k == 0 ? fma(ar, wr, -__dmul_rn(ai, wi)) : fma(-ai, wi, __dmul_rn(ar, wr));   // next element
        const double bi = fma(ai, wr, __dmul_rn(ar, wi));
        out[k / 2] = make_float4((float)ar, (float)ai, (float)br, (float)bi);
        ar = fma(br, wr, -__dmul_rn(bi, wi));                                                           // the one after
        ai = fma(bi, wr, __dmul_rn(br, wi));
    }
}

__device__ __forceinline__ void steer_chunk(double ang, double wr, double wi, int m0, float4 (&out)[kGeoChunk / 2]) {
    const double2 z = steer_head(ang, m0);
    steer_chunk_from_head(z.x, z.y, wr, wi, out);
}

}  // namespace risvec
