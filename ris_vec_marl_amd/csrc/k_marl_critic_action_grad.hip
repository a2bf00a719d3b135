// d min(q1, q2) / d action of the multi-agent (SAC) learner's actor update (Global_SAC_Critic.centralized_actor_update,
// Simulation-MARL-BCD/global_sac_critic.py:174-176 and the backward() at :246) without an autograd graph, in TWO launches,
// for n rows and n_nets in {1, 2} CriticNetworks (networks.py:38-49) of one shape, per row b and net c:
//     x = [state | action]   h1, h2, h3, q_c: the forward walk of k_marl_critic (the same bits)
//     d3 = wq * [h3 > 0]     d2 = (W3^T d3) * [h2 > 0]     d1 = (W2^T d2) * [h1 > 0]
//     g_c[b, :] = (W1^T d1)[S : S + A]
//     w_1, w_2 = (1, 0) if q1 < q2, (0, 1) if q1 > q2, (0.5, 0.5) if q1 == q2        torch.min's backward; one net: w = 1
//     out[b, :] = scale (w_1 g_1[b, :] + w_2 g_2[b, :])          q_min[b] = min(q1, q2)
// No weight gradient is formed and no activation leaves the workgroup.  Orientation, precision and register order are those
// of risvec_mfma.hpp; the forward is the walk of risvec_critic_walk.hpp, the transposed products and the scaling of the
// deltas are those of risvec_critic_grad.hpp, as in k_marl_critic_grad.hip.
//
// 1  k_marl_critic_action_grad_rows<MT2, MT3>: grid (32-row tiles, nets), four wavefronts per tile.
//    Forward: marl_stage_input, critic_fc1_walk, critic_fc2 and an fc3 block that keeps its tiles for d3.  The lane that
//    produces an activation tile keeps [y > 0] of its 16 values as 16 bits in registers: h1's in two 64-bit words (group
//    wave + 4 k at bits 16 k; NG <= 32, so k < 8), h2's in one (tile wave MT2 + m at bits 16 m).  The same lane owns the same
//    tile in the backward, so no activation is written anywhere.
//    d3 -> d2 -> d1 as in k_marl_critic_grad_rows: gemm_tiles_t on W3 / W2 read in place, times the power of two of the
//    stream's `scales`; a tile's deltas are multiplied into [64, 128) before the float16 split and the accumulator is
//    multiplied back.
//    W1^T d1: the wavefront that finishes d1 group g scales that one tile by its own power of two, leaves it as B fragments
//    in a private slot of 2 k-steps -- s_h k-steps [K3 + 2 wave, K3 + 2 wave + 2), where d3 lay; d2's fragments stay in
//    [0, K3) -- and multiplies it into its own accumulators of the ceil(A / 32) <= 4 output tiles: the A operand of lane
//    (i, h) at k-step s is W1[32 g + 16 s + 8 (j >> 2) + 4 h + (j & 3)][S + min(32 m + i, A - 1)], j = 0..7.  The column is
//    CLAMPED: a column at or beyond S + A is never read, and the clamped lanes' output rows are never stored.  Then the
//    four wavefronts' partial tiles meet through LDS ([4][32][33] floats at the start of the dynamic LDS, everything there
//    being dead) and are added in wavefront order, one output tile at a time.
//    Workspace, float32, npad = n rounded up to 32, per net: g_c [npad][A], q_c [npad].  Rows >= n of the last tile walk row
//    0's input; no state or action row >= n is read.
//    LDS: that of k_marl_critic_grad_rows at the same shape.  Scratch: 0.
//
// 2  k_marl_critic_action_grad_select: one thread per element of out [n][A]; rows >= n are not written.
//
// Every barrier sits under wave-uniform control flow.  No global address depends on loaded data.  No atomics: every call gives
// the same bits.
#include "risvec_critic_grad.hpp"
#include "risvec_critic_walk.hpp"
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"

namespace risvec {
namespace {

constexpr int kActTiles = 4;         // output tiles of 32 action columns: A <= 127
constexpr int kStagePitch = 33;      // floats per column of a staged tile: 32 rows + 1, so both sides stay off bank conflicts

struct ActNetPtrs {
    MarlNetPtrs fwd;
    const float* W1;               // [F1, S + A]
    const float* W2;               // [F2, F1]
    const float* W3;               // [F3, F2]
    float* g;                      // [npad][A]
    float* qw;                     // [npad]: the workspace copy of q
    float* q;                      // [n_rows] or NULL
};

struct ActRowArgs {
    int n_rows, S, NA, KS, NG, F1, F2, MTA;
    const float* state;
    const float* action;
    ActNetPtrs net[2];
};

// [y > 0] of a C/D tile's 16 values, bit q = register q
__device__ __forceinline__ unsigned long long mask16(const f32x16_t& y) {
    unsigned int b = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) b |= (y[q] > 0.0f ? 1u : 0u) << q;
    return b;
}

// y * [bit q of bits] * mult
__device__ __forceinline__ void apply_mask(f32x16_t& y, unsigned int bits, float mult) {
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] = (bits >> q) & 1u ? y[q] * mult : 0.0f;
}

// LDS writes of this wavefront become visible to its own later reads (and the reverse): the slot of W1^T d1 is private to
// the wavefront, so no workgroup barrier is needed
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_marl_critic_action_grad_rows(ActRowArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    constexpr int K4 = 8 * MT3;                               // k-steps of d3 = fc3 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int KS = A.KS, NG = A.NG;
    const int netc = blockIdx.y;                              // uniform over the workgroup
    const ActNetPtrs& G = A.net[netc];
    const MarlNetPtrs& P = G.fwd;
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(2 NG, K3 + K4)][2][64]
    const int hsteps = max(2 * NG, K3 + K4);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    float* s_max = s_red + kCriticWaves * 32;                     // slot 1 of s_red: [2][4] maxima
    uint4* s_d3 = s_h + K3 * 2 * kWave;                       // the d3 fragments, beside h2's; then the wavefronts' d1 slots
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32, col = e0 + r;

    marl_stage_input(A.state, A.action, A.S, A.NA, A.n_rows, s_in, e0, 0, KS, tid);
    __syncthreads();

    const float u1 = P.scales[0], u2 = P.scales[1], u3 = P.scales[2];
    unsigned long long m1lo = 0, m1hi = 0, m2 = 0;            // the ReLU masks of this lane's h1 and h2 tiles
    // ---- fc1: bias, ReLU, the split fragments to LDS, the mask to registers
    critic_fc1_walk(P.ws + L.fc1 * kWave, s_in, KS, NG, wave, lane, [&](int g, const f32x16_t& d) {
        const f32x16_t y = bias_relu(d, u1, tile_of(P.b1, 32 * g, h));
        put_tile(s_h, g, y, lane);
        const int k = (g - wave) >> 2;                        // g = wave + 4 k
        const unsigned long long b = mask16(y);
        if (k < 4) m1lo |= b << (16 * k);
        else m1hi |= b << (16 * (k - 4));
    });
    __syncthreads();

    // ---- fc2
    critic_fc2<MT2>(P, s_h, L, NG, wave, lane, u2, [&](int t, const f32x16_t& y) { m2 |= mask16(y) << (16 * (t - wave * MT2)); });

    // ---- fc3 + ReLU, the q dot product, and d3 = wq [h3 > 0] in the registers of the fc3 tiles
    f32x16_t d3[MT3];
    {
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
            const f32x16_t y = bias_relu(a3[m], u3, tile_of(P.b3, f0, h));
            const f32x16_t qw = tile_of(P.qw, f0, h);
            const f32x16_t p = y * qw;
            qs = m == 0 ? p : qs + p;
#pragma unroll
            for (int q = 0; q < 16; ++q) d3[m][q] = y[q] > 0.0f ? qw[q] : 0.0f;
        }
        float qp = sum16(qs);
        qp += __shfl_xor(qp, 32, kWave);
        if (h == 0) s_red[wave * 32 + r] = qp;
    }
    float mx = 0.0f;
#pragma unroll
    for (int m = 0; m < MT3; ++m) mx = absmax16(d3[m], mx);
    mx = wave_max(mx);
    if (lane == 0) s_max[4 + wave] = mx;
    __syncthreads();                                          // every wavefront is past its fc3 MFMAs: h2's fragments are dead

    if (wave == 0 && h == 0) {
        const float qv = marl_red(s_red, 0, r) + P.qb[0];
        G.qw[col] = qv;
        if (G.q && col < A.n_rows) G.q[col] = qv;
    }
    const int s3 = grad_scale_exp(fmaxf(fmaxf(s_max[4], s_max[5]), fmaxf(s_max[6], s_max[7])));
    {
        const float up = ldexpf(1.0f, s3);
#pragma unroll
        for (int m = 0; m < MT3; ++m) put_tile(s_d3, wave * MT3 + m, d3[m] * up, lane);
    }
    __syncthreads();

    // ---- d2 = (W3^T d3) [h2 > 0]: the fc2 tiles this wavefront owned in the forward
    int s2;
    {
        f32x16_t acc[MT2];
#pragma unroll
        for (int m = 0; m < MT2; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
        gemm_tiles_t<MT2>(acc, G.W3, A.F2, 32 * wave * MT2, 1.0f / u3, s_d3, K4, lane);
        const float back = u3 * ldexpf(1.0f, -s3);
        mx = 0.0f;
#pragma unroll
        for (int m = 0; m < MT2; ++m) {
            apply_mask(acc[m], (unsigned int)(m2 >> (16 * m)), back);
            mx = absmax16(acc[m], mx);
        }
        mx = wave_max(mx);
        if (lane == 0) s_max[wave] = mx;
        __syncthreads();                                      // and every wavefront is past its reads of d3
        s2 = grad_scale_exp(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])));
        const float up = ldexpf(1.0f, s2);
#pragma unroll
        for (int m = 0; m < MT2; ++m) put_tile(s_h, wave * MT2 + m, acc[m] * up, lane);
        __syncthreads();
    }

    // ---- d1 = (W2^T d2) [h1 > 0], fc1 groups wave, wave + 4, .., each multiplied through W1^T's action columns at once
    f32x16_t ga[kActTiles];
#pragma unroll
    for (int m = 0; m < kActTiles; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) ga[m][q] = 0.0f;
    {
        const float back1 = u2 * ldexpf(1.0f, -s2);
        const int ld = A.S + A.NA;
        uint4* slot = s_d3 + (2 * wave) * 2 * kWave;          // this wavefront's 2 k-steps
        int k = 0;
        for (int g = wave; g < NG; g += kCriticWaves, ++k) {
            f32x16_t a1[1];
#pragma unroll
            for (int q = 0; q < 16; ++q) a1[0][q] = 0.0f;
            gemm_tiles_t<1>(a1, G.W2, A.F1, 32 * g, 1.0f / u2, s_h, K3, lane);
            apply_mask(a1[0], (unsigned int)(k < 4 ? m1lo >> (16 * k) : m1hi >> (16 * (k - 4))), back1);
            const int s1 = grad_scale_exp(wave_max(absmax16(a1[0], 0.0f)));
            put_tile(slot, 0, a1[0] * ldexpf(1.0f, s1), lane);
            wave_lds_sync();
            half8_t bh[2], bl[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bh[s] = ld_frag(slot + (2 * s) * kWave + lane);
                bl[s] = ld_frag(slot + (2 * s + 1) * kWave + lane);
            }
            wave_lds_sync();                                  // the slot is free for the next group
            const float back0 = u1 * ldexpf(1.0f, -s1), mult = 1.0f / u1;
            const float* w1g = G.W1 + (size_t)(32 * g + 4 * h) * ld + A.S;
#pragma unroll
            for (int m = 0; m < kActTiles; ++m) {
                if (m < A.MTA) {                              // uniform over the workgroup
                    const float* w = w1g + min(32 * m + r, A.NA - 1);     // never a column at or beyond S + A
                    f32x16_t t;
#pragma unroll
                    for (int q = 0; q < 16; ++q) t[q] = 0.0f;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        f32x8_t wv;
#pragma unroll
                        for (int j = 0; j < 8; ++j) wv[j] = w[(size_t)(16 * s + 8 * (j >> 2) + (j & 3)) * ld];
                        half8_t ah, al;
                        split16(wv * mult, ah, al);
                        t = mfma3(ah, al, bh[s], bl[s], t);
                    }
                    ga[m] += t * back0;
                }
            }
        }
    }
    __syncthreads();                                          // every wavefront is past d2's fragments: the LDS is free

    // ---- the four partial tiles of output tile m, added in wavefront order -> g [npad][A]
    float* s_st = reinterpret_cast<float*>(s_mem);            // [4][32][kStagePitch]
#pragma unroll
    for (int m = 0; m < kActTiles; ++m) {
        if (m < A.MTA) {                                      // uniform over the workgroup
#pragma unroll
            for (int q = 0; q < 16; ++q) s_st[(wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * h) * kStagePitch + r] = ga[m][q];
            __syncthreads();
            for (int idx = tid; idx < 32 * 32; idx += kMcBlock) {
                const int rr = idx >> 5, cl = idx & 31, c = 32 * m + cl;
                if (c < A.NA) {
                    const float* p = s_st + cl * kStagePitch + rr;
                    G.g[(size_t)(e0 + rr) * A.NA + c] =
                        ((p[0] + p[32 * kStagePitch]) + p[2 * 32 * kStagePitch]) + p[3 * 32 * kStagePitch];
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct ActSelArgs {
    long long total;                                          // n_rows A
    int NA, n_nets;
    float scale;
    const float* g1; const float* g2; const float* q1; const float* q2;
    float* out;                                               // [n_rows][A]
    float* q_min;                                             // [n_rows] or NULL
};

constexpr int kSelBlock = 256;

__global__ void __launch_bounds__(kSelBlock)
k_marl_critic_action_grad_select(ActSelArgs A) {
    const long long idx = (long long)blockIdx.x * kSelBlock + threadIdx.x;
    if (idx >= A.total) return;
    const long long b = idx / A.NA;
    float g = A.g1[idx], qm = A.q1[b];
    if (A.n_nets == 2) {
        const float q1 = qm, q2 = A.q2[b], g2 = A.g2[idx];
        g = q1 < q2 ? g : (q1 > q2 ? g2 : 0.5f * (g + g2));
        qm = (q1 < q2 || q1 != q1) ? q1 : q2;                 // torch.minimum: a NaN stays
    }
    A.out[idx] = A.scale * g;
    if (A.q_min && idx == b * A.NA) A.q_min[b] = qm;
}

inline long long round32(long long v) { return (v + 31) / 32 * 32; }

inline long long act_net_floats(long long npad, int A) { return npad * A + npad; }

}  // namespace

bool marl_critic_action_grad_supported(int S, int A, int F1, int F2, int F3) { return marl_critic_supported(S, A, F1, F2, F3); }

size_t marl_critic_action_grad_workspace(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets) {
    if (n_rows < 1 || n_nets < 1 || n_nets > 2 || !marl_critic_action_grad_supported(S, A, F1, F2, F3)) return 0;
    return (size_t)(n_nets * act_net_floats(round32(n_rows), A)) * sizeof(float);
}

hipError_t launch_marl_critic_action_grad(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets,
                                          const RisVecMarlCriticActionGradNet* nets, const float* state, const float* action, float scale,
                                          float* q1, float* q2, float* q_min, float* out, void* workspace, hipStream_t st) {
    if (!marl_critic_action_grad_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2 || n_rows < 1) return hipErrorInvalidValue;
    const long long npad = round32(n_rows), ntiles = npad / 32;
    const int MT2 = F2 / 128, MT3 = F3 / 128;
    ActRowArgs r{};
    r.n_rows = (int)n_rows; r.S = S; r.NA = A; r.KS = ks_of(S + A); r.NG = F1 / 32; r.F1 = F1; r.F2 = F2; r.MTA = (A + 31) / 32;
    r.state = state; r.action = action;
    float* p = static_cast<float*>(workspace);
    for (int c = 0; c < 2; ++c) {
        const int k = c < n_nets ? c : 0;                     // a single net fills both slots
        ActNetPtrs& g = r.net[c];
        float* b = p + (size_t)k * act_net_floats(npad, A);
        g.fwd = marl_net_ptrs(nets[k].fwd); g.W1 = nets[k].W1; g.W2 = nets[k].W2; g.W3 = nets[k].W3;
        g.g = b; g.qw = b + (size_t)npad * A;
        g.q = k == 0 ? q1 : q2;
    }
    note_kernel("k_marl_critic_action_grad_rows<%d,%d>x%d -> k_marl_critic_action_grad_select", MT2, MT3, n_nets);
    const size_t lds = (size_t)(r.KS + std::max(2 * r.NG, 8 * MT2 + 8 * MT3)) * 2 * kWave * sizeof(uint4) +
                       (size_t)kRedSlots * kCriticWaves * 32 * sizeof(float);
    hipError_t err = dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) {
        return launch_dynamic_lds(k_marl_critic_action_grad_rows<decltype(mt2)::value, decltype(mt3)::value>,
                                  dim3((unsigned)ntiles, (unsigned)n_nets), dim3(kMcBlock), lds, st, r);
    });
    if (err != hipSuccess) return err;
    ActSelArgs s{};
    s.total = n_rows * A; s.NA = A; s.n_nets = n_nets; s.scale = scale;
    s.g1 = r.net[0].g; s.g2 = r.net[1].g; s.q1 = r.net[0].qw; s.q2 = r.net[1].qw; s.out = out; s.q_min = q_min;
    hipLaunchKernelGGL(k_marl_critic_action_grad_select, dim3((unsigned)((s.total + kSelBlock - 1) / kSelBlock)), dim3(kSelBlock), 0, st, s);
    return hipGetLastError();
}

}  // namespace risvec
