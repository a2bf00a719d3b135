// The walk of one plain ReLU CriticNetwork (Simulation-MARL-BCD/networks.py:38-49) by a workgroup of four wavefronts on
// one tile of 32 rows, as k_marl_critic.hip's header describes it: what k_marl_critic (the global twin critic) and
// k_local_critics (every agent's local twin critic) both instantiate.  The two kernels differ in where the input comes
// from, in which net a workgroup walks and in the epilogue; the input-fragment store, the net walk and the reduction of the
// q partial sums exist here, once.  Orientation, precision and register order are those of risvec_mfma.hpp.
//
// LDS, carved by the kernel (marl_walk_lds_bytes):
//   s_in  the split B fragments of the input x, staged ONCE for all nets     [KS k-steps][hi | lo][64 lanes] x 16 bytes
//   s_h   the fc1 activations, then the fc2 activations (each dead before the next)  [max(2 NG, fc2 / 16)][hi | lo][64]
//   s_red the per-row partial sums of the q dot product, one slot per net: [kRedSlots][4 waves][32]
// k_marl_critic_wide carves the same three with an s_in of 8 k-steps that it restages chunk by chunk; it runs fc1 itself
// and takes the rest of the walk from marl_run_tail.
#pragma once

#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"

namespace risvec {

struct MarlNetPtrs {
    const uint4* ws;               // the weight stream: fragment rows of 64 x 16 bytes
    const float* scales;           // [3] undo the fc1, fc2 and fc3 weight scalings
    const float* b1;               // [F1]
    const float* b2;               // [F2]
    const float* b3;               // [F3]
    const float* qw;               // [F3]
    const float* qb;               // [1]
};

inline MarlNetPtrs marl_net_ptrs(const RisVecMarlCriticNet& n) {
    return MarlNetPtrs{static_cast<const uint4*>(n.wstream), n.scales, n.b1, n.b2, n.b3, n.qw, n.qb};
}

constexpr int kMcBlock = 256;        // 4 wavefronts = 1 per SIMD, all on the same 32 rows
constexpr int kMcWaves = kCriticWaves;
constexpr int kRedSlots = 2;

inline size_t marl_walk_lds_bytes(int KS, int NG, int MT2) {
    const int hsteps = std::max(2 * NG, 8 * MT2);
    return (size_t)(KS + hsteps) * 2 * kWave * sizeof(uint4) + (size_t)kRedSlots * kMcWaves * 32 * sizeof(float);
}

// The 8 input values x[16 s + 8 h + j] of lane l = (r, h) -> the split B fragments of k-step s
__device__ __forceinline__ void put_input(uint4* s_in, int s, int l, const f32x8_t& v) {
    half8_t hi, lo;
    split16(v, hi, lo);
    s_in[(2 * s) * kWave + l] = __builtin_bit_cast(uint4, hi);
    s_in[(2 * s + 1) * kWave + l] = __builtin_bit_cast(uint4, lo);
}

// One net: fc1 -> s_h, fc2 -> s_h, fc3 and the q dot product -> s_red[slot].  Called under wave-uniform control flow;
// ends on a barrier, after which s_h is free again and s_red[slot] is complete.
template <int MT2, int MT3>
__device__ __forceinline__ void marl_run_net(const MarlNetPtrs& P, int slot, const uint4* s_in, uint4* s_h, float* s_red,
                                             const MarlLayout& L, int KS, int NG, int wave, int lane) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    const int r = lane & 31, h = lane >> 5;
    const float u1 = P.scales[0], u2 = P.scales[1], u3 = P.scales[2];
    // ---- fc1, groups wave, wave + 4, .. (the group walk is the twin of k_sarl_critic.hip's; keep the two in step): bias,
    // ReLU, and the split fragments of the group's 32 features go to LDS
    const int ngw = NG > wave ? (NG - wave + kMcWaves - 1) / kMcWaves : 0;
    if (ngw > 0) {                                            // wave-uniform; no barrier inside
        const int nst = ngw * KS;
        const uint4* w1 = P.ws + L.fc1 * kWave + lane;
        half8_t ah[kAhead], al[kAhead];
        int fg = wave, fs = 0;                                // (group, k-step) of the next fetch
        auto fetch = [&](int i) {
            const uint4* p = w1 + (size_t)(fg * KS + fs) * (2 * kWave);
            ah[i] = ld_frag(p);
            al[i] = ld_frag(p + kWave);
            if (fs + 1 < KS) ++fs;
            else if (fg + kMcWaves < NG) { fg += kMcWaves; fs = 0; }    // else: stay on the last fragment
        };
#pragma unroll
        for (int i = 0; i < kAhead; ++i) fetch(i);
        f32x16_t d;
#pragma unroll
        for (int q = 0; q < 16; ++q) d[q] = 0.0f;
        int g = wave, s = 0;
        for (int i0 = 0; i0 < nst; i0 += kAhead) {
#pragma unroll
            for (int i = 0; i < kAhead; ++i) {
                if (i0 + i < nst) {
                    const half8_t bh = ld_frag(s_in + (2 * s) * kWave + lane), bl = ld_frag(s_in + (2 * s + 1) * kWave + lane);
                    d = mfma3(ah[i], al[i], bh, bl, d);
                    fetch(i);
                    if (++s == KS) {
                        put_tile(s_h, g, bias_relu(d, u1, tile_of(P.b1, 32 * g, h)), lane);
#pragma unroll
                        for (int q = 0; q < 16; ++q) d[q] = 0.0f;
                        s = 0;
                        g += kMcWaves;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- fc2: output tiles [wave MT2, (wave + 1) MT2) over all 2 NG k-steps
    f32x16_t acc[MT2];
#pragma unroll
    for (int m = 0; m < MT2; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
    gemm_tiles<MT2>(acc, P.ws + (L.fc2 + (long long)wave * (2 * NG) * MT2 * 2) * kWave, s_h, 2 * NG, lane);
    __syncthreads();                                          // every wavefront is past its fc2 MFMAs: s_h is free
#pragma unroll
    for (int m = 0; m < MT2; ++m) {
        const int t = wave * MT2 + m;
        put_tile(s_h, t, bias_relu(acc[m], u2, tile_of(P.b2, 32 * t, h)), lane);
    }
    __syncthreads();

    // ---- fc3 + ReLU, then the 1-wide q layer as a dot product in registers
    f32x16_t a3[MT3];
#pragma unroll
    for (int m = 0; m < MT3; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) a3[m][q] = 0.0f;
    gemm_tiles<MT3>(a3, P.ws + (L.fc3 + (long long)wave * K3 * MT3 * 2) * kWave, s_h, K3, lane);
    f32x16_t qs;
#pragma unroll
    for (int m = 0; m < MT3; ++m) {
        const int f0 = 32 * (wave * MT3 + m);
        const f32x16_t p = bias_relu(a3[m], u3, tile_of(P.b3, f0, h)) * tile_of(P.qw, f0, h);
        qs = m == 0 ? p : qs + p;
    }
    float qp = sum16(qs);
    qp += __shfl_xor(qp, 32, kWave);
    if (h == 0) s_red[(slot * kMcWaves + wave) * 32 + r] = qp;
    __syncthreads();                                          // every wavefront is past its fc3 MFMAs: s_h is free
}

// marl_run_net from its second barrier on, for a kernel that runs fc1 its own way (k_marl_critic_wide): the fc1
// activations in s_h -> fc2 -> s_h, fc3 and the q dot product -> s_red[slot]; u2, u3 undo the fc2 and fc3 weight scalings.
// Called under wave-uniform control flow after the barrier that completes s_h; ends on a barrier, after which s_h is free
// again and s_red[slot] is complete.  A RESTATEMENT of marl_run_net's second half, statement for statement: having
// marl_run_net call it changes k_marl_critic<4, *>'s registers (160 -> 162 VGPRs).  Keep the two in step.
template <int MT2, int MT3>
__device__ __forceinline__ void marl_run_tail(const MarlNetPtrs& P, int slot, uint4* s_h, float* s_red, const MarlLayout& L, int NG,
                                              int wave, int lane, float u2, float u3) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    const int r = lane & 31, h = lane >> 5;
    // ---- fc2: output tiles [wave MT2, (wave + 1) MT2) over all 2 NG k-steps
    f32x16_t acc[MT2];
#pragma unroll
    for (int m = 0; m < MT2; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
    gemm_tiles<MT2>(acc, P.ws + (L.fc2 + (long long)wave * (2 * NG) * MT2 * 2) * kWave, s_h, 2 * NG, lane);
    __syncthreads();                                          // every wavefront is past its fc2 MFMAs: s_h is free
#pragma unroll
    for (int m = 0; m < MT2; ++m) {
        const int t = wave * MT2 + m;
        put_tile(s_h, t, bias_relu(acc[m], u2, tile_of(P.b2, 32 * t, h)), lane);
    }
    __syncthreads();

    // ---- fc3 + ReLU, then the 1-wide q layer as a dot product in registers
    f32x16_t a3[MT3];
#pragma unroll
    for (int m = 0; m < MT3; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) a3[m][q] = 0.0f;
    gemm_tiles<MT3>(a3, P.ws + (L.fc3 + (long long)wave * K3 * MT3 * 2) * kWave, s_h, K3, lane);
    f32x16_t qs;
#pragma unroll
    for (int m = 0; m < MT3; ++m) {
        const int f0 = 32 * (wave * MT3 + m);
        const f32x16_t p = bias_relu(a3[m], u3, tile_of(P.b3, f0, h)) * tile_of(P.qw, f0, h);
        qs = m == 0 ? p : qs + p;
    }
    float qp = sum16(qs);
    qp += __shfl_xor(qp, 32, kWave);
    if (h == 0) s_red[(slot * kMcWaves + wave) * 32 + r] = qp;
    __syncthreads();                                          // every wavefront is past its fc3 MFMAs: s_h is free
}

// Row r's q dot product of the net in `slot`: the four wavefronts' partial sums in wavefront order
__device__ __forceinline__ float marl_red(const float* s_red, int slot, int r) {
    const float* p = s_red + slot * kMcWaves * 32 + r;
    return ((p[0] + p[32]) + p[64]) + p[96];
}

}  // namespace risvec
