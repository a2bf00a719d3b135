// What the backward walks of the critic kernels share (k_marl_critic_grad.hip, k_marl_critic_action_grad.hip): the
// transposed product on float32 weights read in place, and the power-of-two scaling of the deltas around the float16
// split.  Orientation, precision and register order are those of risvec_mfma.hpp.
#pragma once

#include "risvec_mfma.hpp"

namespace risvec {

constexpr int kGradScaleClamp = 80;  // |s| of the 2^s a delta is scaled by

// the largest entry of a tile / layer -> s with amax 2^s in [64, 128), clamped
__device__ __forceinline__ int grad_scale_exp(float amax) {
    int ex;
    (void)frexpf(fmaxf(amax, 1e-30f), &ex);                   // amax = m 2^ex, m in [0.5, 1)
    return min(max(7 - ex, -kGradScaleClamp), kGradScaleClamp);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

__device__ __forceinline__ float absmax16(const f32x16_t& y, float m) {
#pragma unroll
    for (int q = 0; q < 16; ++q) m = fmaxf(m, fabsf(y[q]));
    return m;
}

// acc[m] += (W^T)_m . B over nks k-steps: W [K][ld] float32 in place, output tile m = columns [i0 + 32 m, i0 + 32 m + 32) of
// W, k in the permuted order of put_tile; sb: the B fragments in LDS, [nks][hi | lo][64].  As in gemm_tiles the loads run
// kAhead k-steps ahead of their MFMAs, and the prefetch index is clamped to the last k-step.  nks >= 1.
template <int MT>
__device__ __forceinline__ void gemm_tiles_t(f32x16_t (&acc)[MT], const float* __restrict__ W, int ld, int i0, float mult, const uint4* sb,
                                             int nks, int lane) {
    const int i = lane & 31, h = lane >> 5;
    const float* w0 = W + i0 + i;
    f32x8_t wv[kAhead][MT];
    auto fetch = [&](int slot, int s) {
        const int sc = s < nks ? s : nks - 1;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[slot][m][j] = w0[(size_t)(16 * sc + 8 * (j >> 2) + 4 * h + (j & 3)) * ld + 32 * m];
    };
#pragma unroll
    for (int a = 0; a < kAhead; ++a) fetch(a, a);
    for (int s0 = 0; s0 < nks; s0 += kAhead) {
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            const int s = s0 + a;
            if (s < nks) {
                const half8_t bh = ld_frag(sb + (2 * s) * kWave + lane), bl = ld_frag(sb + (2 * s + 1) * kWave + lane);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    half8_t ah, al;
                    split16(wv[a][m] * mult, ah, al);
                    acc[m] = mfma3(ah, al, bh, bl, acc[m]);
                }
                fetch(a, s + kAhead);
            }
        }
    }
}

}  // namespace risvec
