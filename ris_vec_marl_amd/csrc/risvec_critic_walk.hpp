// The critic walk: how a workgroup of four wavefronts takes one tile of 32 rows through a critic MLP, as
// k_marl_critic.hip's header describes it.  This is the one place where its pieces exist; every critic kernel
// instantiates them from here and adds only what it does differently:
//   marl_stage_input  [state | action | 0 ..] -> split B fragments      k_marl_critic, k_marl_critic_wide, ..._grad_rows,
//                                                                       ..._action_grad_rows (as every ..._grad_rows line below)
//   critic_fc1_walk   the fc1 group walk, a callback per finished group k_sarl_critic, ..._grad_rows, marl_run_net
//   critic_fc2        fc2 -> bias, ReLU -> s_h, a tap per output tile   ..._grad_rows, marl_run_tail
//   critic_fc3_q      fc3, ReLU, the q dot product -> s_red[slot]       marl_run_tail
//   marl_run_tail     critic_fc2 + critic_fc3_q                         k_marl_critic_wide (after its chunked fc1)
//   marl_run_net      critic_fc1_walk + marl_run_tail: one plain ReLU CriticNetwork (Simulation-MARL-BCD/networks.py:38-49)
//                                                                       k_marl_critic, k_local_critics
//   marl_red          the four wavefronts' partial sums of a row        all of them
// Orientation, precision and register order are those of risvec_mfma.hpp.
//
// LDS, carved by the kernel (marl_walk_lds_bytes):
//   s_in  the split B fragments of the input x, staged ONCE for all nets     [KS k-steps][hi | lo][64 lanes] x 16 bytes
//   s_h   the fc1 activations, then the fc2 activations (each dead before the next)  [max(2 NG, fc2 / 16)][hi | lo][64]
//   s_red the per-row partial sums of the q dot product, one slot per net: [kRedSlots][4 waves][32]
// k_marl_critic_wide carves the same three with an s_in of 8 k-steps that it restages chunk by chunk.
//
// Every function here is called under wave-uniform control flow.  The callbacks (on_group, tap) run inside the walk,
// between its barriers, some of them under a wave-uniform guard that not every wavefront passes: a callback MUST NOT
// contain a barrier.
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

constexpr int kMcBlock = kCriticWaves * kWave;   // 4 wavefronts = 1 per SIMD, all on the same 32 rows
constexpr int kRedSlots = 2;

inline size_t marl_walk_lds_bytes(int KS, int NG, int MT2) {
    const int hsteps = std::max(2 * NG, 8 * MT2);
    return (size_t)(KS + hsteps) * 2 * kWave * sizeof(uint4) + (size_t)kRedSlots * kCriticWaves * 32 * sizeof(float);
}

// The 8 input values x[16 s + 8 h + j] of lane l = (r, h) -> the split B fragments of k-step s
__device__ __forceinline__ void put_input(uint4* s_in, int s, int l, const f32x8_t& v) {
    half8_t hi, lo;
    split16(v, hi, lo);
    s_in[(2 * s) * kWave + l] = __builtin_bit_cast(uint4, hi);
    s_in[(2 * s + 1) * kWave + l] = __builtin_bit_cast(uint4, lo);
}

// The split B fragments of k-steps [s0, s0 + ns) of the tile's input -> s_in[0 .. ns): k-step s, lane (r, h) holds
// x[16 s + 8 h + j], j < 8; x = [state | action | 0 ..].  Rows at or beyond n_rows read row 0.  No barrier.
__device__ __forceinline__ void marl_stage_input(const float* state, const float* action, int S, int NA, long long n_rows, uint4* s_in,
                                                 long long e0, int s0, int ns, int tid) {
    const int W = S + NA;
    for (int idx = tid; idx < ns * kWave; idx += kMcBlock) {
        const int s = idx >> 6, l = idx & 63, rr = l & 31, hh = l >> 5;
        const long long row = e0 + rr < n_rows ? e0 + rr : 0;
        const float* ps = state + row * S;
        const float* pa = action + row * NA;
        f32x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * (s0 + s) + 8 * hh + j;
            v[j] = k < S ? ps[k] : (k < W ? pa[k - S] : 0.0f);
        }
        put_input(s_in, s, l, v);
    }
}

// The fc1 group walk: this wavefront's groups wave, wave + 4, .. of 32 output features, each over the KS k-steps of s_in.
// w1: the fc1 block of the weight stream, [NG][KS][hi | lo][64].  The weight fragments go L2 -> registers kAhead k-steps
// ahead of their MFMAs, across group boundaries; the prefetch stays on the last fragment once it has reached it.
// on_group(g, d) receives group g's raw accumulator (weight scaling not undone).  No barrier inside, and none in on_group.
template <class OnGroup>
__device__ __forceinline__ void critic_fc1_walk(const uint4* w1, const uint4* s_in, int KS, int NG, int wave, int lane, OnGroup&& on_group) {
    const int ngw = NG > wave ? (NG - wave + kCriticWaves - 1) / kCriticWaves : 0;
    if (ngw > 0) {                                            // wave-uniform
        const int nst = ngw * KS;
        w1 += lane;
        half8_t ah[kAhead], al[kAhead];
        int fg = wave, fs = 0;                                // (group, k-step) of the next fetch
        auto fetch = [&](int i) {
            const uint4* p = w1 + (size_t)(fg * KS + fs) * (2 * kWave);
            ah[i] = ld_frag(p);
            al[i] = ld_frag(p + kWave);
            if (fs + 1 < KS) ++fs;
            else if (fg + kCriticWaves < NG) { fg += kCriticWaves; fs = 0; }    // else: stay on the last fragment
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
                        on_group(g, d);
#pragma unroll
                        for (int q = 0; q < 16; ++q) d[q] = 0.0f;
                        s = 0;
                        g += kCriticWaves;
                    }
                }
            }
        }
    }
}

// what critic_fc2 does with an output tile beyond leaving it in s_h: nothing
struct NoTap {
    __device__ __forceinline__ void operator()(int, const f32x16_t&) const {}
};

// fc2: the fc1 activations in s_h -> output tiles [wave MT2, (wave + 1) MT2) over all 2 NG k-steps -> bias, ReLU -> s_h.
// tap(t, y) sees tile t's activations as they go to LDS (no barrier in it).  Called after the barrier that completes s_h;
// ends on the barrier that completes it again.
template <int MT2, class Tap = NoTap>
__device__ __forceinline__ void critic_fc2(const MarlNetPtrs& P, uint4* s_h, const MarlLayout& L, int NG, int wave, int lane, float u2,
                                           Tap&& tap = Tap{}) {
    const int h = lane >> 5;
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
        const f32x16_t y = bias_relu(acc[m], u2, tile_of(P.b2, 32 * t, h));
        put_tile(s_h, t, y, lane);
        tap(t, y);
    }
    __syncthreads();
}

// fc3 + ReLU on the fc2 activations in s_h, then the 1-wide q layer as a dot product in registers -> s_red[slot].  Ends on
// a barrier, after which s_h is free again and s_red[slot] is complete.
template <int MT2, int MT3>
__device__ __forceinline__ void critic_fc3_q(const MarlNetPtrs& P, int slot, const uint4* s_h, float* s_red, const MarlLayout& L, int wave,
                                             int lane, float u3) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    const int r = lane & 31, h = lane >> 5;
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
    if (h == 0) s_red[(slot * kCriticWaves + wave) * 32 + r] = qp;
    __syncthreads();                                          // every wavefront is past its fc3 MFMAs: s_h is free
}

// The walk from the fc1 activations on: s_h -> fc2 -> s_h, fc3 and the q dot product -> s_red[slot]; u2, u3 undo the fc2
// and fc3 weight scalings.  Called after the barrier that completes s_h; ends on a barrier, after which s_h is free again
// and s_red[slot] is complete.
template <int MT2, int MT3>
__device__ __forceinline__ void marl_run_tail(const MarlNetPtrs& P, int slot, uint4* s_h, float* s_red, const MarlLayout& L, int NG,
                                              int wave, int lane, float u2, float u3) {
    critic_fc2<MT2>(P, s_h, L, NG, wave, lane, u2);
    critic_fc3_q<MT2, MT3>(P, slot, s_h, s_red, L, wave, lane, u3);
}

// One net: fc1 -> s_h, fc2 -> s_h, fc3 and the q dot product -> s_red[slot].  Ends on a barrier, after which s_h is free
// again and s_red[slot] is complete.
template <int MT2, int MT3>
__device__ __forceinline__ void marl_run_net(const MarlNetPtrs& P, int slot, const uint4* s_in, uint4* s_h, float* s_red,
                                             const MarlLayout& L, int KS, int NG, int wave, int lane) {
    const int h = lane >> 5;
    const float u1 = P.scales[0], u2 = P.scales[1], u3 = P.scales[2];
    // bias, ReLU, and the split fragments of the group's 32 features go to LDS
    critic_fc1_walk(P.ws + L.fc1 * kWave, s_in, KS, NG, wave, lane,
                    [&](int g, const f32x16_t& d) { put_tile(s_h, g, bias_relu(d, u1, tile_of(P.b1, 32 * g, h)), lane); });
    __syncthreads();
    marl_run_tail<MT2, MT3>(P, slot, s_h, s_red, L, NG, wave, lane, u2, u3);
}

// Row r's q dot product of the net in `slot`: the four wavefronts' partial sums in wavefront order
__device__ __forceinline__ float marl_red(const float* s_red, int slot, int r) {
    const float* p = s_red + slot * kCriticWaves * 32 + r;
    return ((p[0] + p[32]) + p[64]) + p[96];
}

}  // namespace risvec
