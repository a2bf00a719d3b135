// The multi-agent (SAC) learner's first step on a sampled batch: the twin target critics of Global_SAC_Critic.global_learn
// (Simulation-MARL-BCD/global_sac_critic.py:338-352) -- each a CriticNetwork.forward (networks.py:38-49), a plain ReLU MLP
// on cat([state, action]) -- and the TD target, in ONE kernel, for n_rows rows and n_nets in {1, 2} weight sets of one shape:
//     x   = [state[row] | action[row]]                     two pointers, read in place
//     h1  = relu(W1 x + b1);  h2 = relu(W2 h1 + b2);  h3 = relu(W3 h2 + b3);  q = wq . h3 + bq        per net
//     m   = n_nets == 2 ? min(q_1, q_2) : q_1
//     ent = coef[0] logp_power[row] + coef[1] logp_intent[row]          a term whose logp pointer is NULL is absent
//     y   = done ? reward : reward + gamma (m - ent)                    a select, as target[done] = rewards_g[done] is
// Orientation, precision and register order are those of risvec_mfma.hpp (read its header).  There is no LayerNorm, so
// fc1 needs neither centring nor a bias row.
//
// The FORM is that of k_sarl_critic: a workgroup of four wavefronts shares ONE tile of 32 rows and splits the OUTPUT
// FEATURES of every layer four ways: wavefront w owns fc1 groups w, w + 4, .. and output tiles [w MT, (w + 1) MT) of fc2 /
// fc3 (MT = features / 128).  A weight fragment is used by exactly one wavefront of the workgroup, so it goes L2 ->
// registers with plain global loads, four k-steps ahead of its MFMAs, and LDS holds what IS shared:
//   s_in  the split B fragments of the input x, staged ONCE for both nets   [KS k-steps][hi | lo][64 lanes] x 16 bytes
//   s_h   the fc1 activations, then the fc2 activations (each dead before the next)  [max(2 NG, fc2 / 16)][hi | lo][64]
//   s_red the per-row partial sums of the q dot product, one slot per net: [2][4 waves][32]
// A lane leaves its C/D tile in LDS as two k-steps (registers 8u .. 8u+7 = k-step u, the permuted k order of the actor)
// and every wavefront reads them back as B operands with one ds_read_b128 per fragment.  The workgroup walks the nets
// one after the other, keeps q_1 in its s_red slot and finishes with the epilogue.
//
// The input staging and the net walk (the fc1 group walk, fc2, fc3, the q dot product, the s_red reduction) are
// risvec_critic_walk.hpp's; this file adds the arguments, the epilogue and the launchers.  k_marl_critic_wide, further
// down, is the same launch for inputs of up to 512 floats: fc1 walks the input in chunks, its own way, between the same
// staging, tail (marl_run_tail) and epilogue.
//
// Every barrier sits under wave-uniform control flow: all loop bounds and the net count come from kernel arguments,
// template parameters and the wavefront index.  Rows at or beyond n_rows are computed on row 0's input and never stored.
// No global address depends on loaded data; every weight prefetch index is clamped to the last fragment of its block.
#include "risvec_critic_walk.hpp"
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"
#include "risvec_step.hpp"

namespace risvec {
namespace {

struct MarlCriticArgs {
    long long n_rows;
    int S, NA, KS, NG, n_nets;     // KS = k-steps of 16 of [state | action]; NG = fc1 / 32
    const float* state;            // [n_rows, S]
    const float* action;           // [n_rows, NA]
    MarlNetPtrs net[2];
    const float* reward;           // [n_rows] or NULL
    const uint8_t* done;           // [n_rows] or NULL
    float gamma;
    const float* coef;             // [2] or NULL
    const float* lp;               // [n_rows] or NULL
    const float* li;               // [n_rows] or NULL
    float* q1;                     // [n_rows] or NULL
    float* q2;                     // [n_rows] or NULL
    float* y;                      // [n_rows] or NULL
};

// The minimum, the entropy term and the target of the tile's rows, from the q partial sums in s_red (after the last net's
// closing barrier)
__device__ __forceinline__ void marl_epilogue(const MarlCriticArgs& A, const float* s_red, long long e0, bool twin, int wave, int lane) {
    const int r = lane & 31, h = lane >> 5;
    if (wave == 0 && h == 0) {
        const long long e = e0 + r;
        if (e < A.n_rows) {
            auto red = [&](int slot) { return marl_red(s_red, slot, r); };
            const float qv1 = red(0) + A.net[0].qb[0];
            float m = qv1;
            if (A.q1) A.q1[e] = qv1;
            if (twin) {
                const float qv2 = red(1) + A.net[1].qb[0];
                if (A.q2) A.q2[e] = qv2;
                m = fminf(qv1, qv2);
            }
            if (A.y) {
                const float rw = A.reward[e];
                float t = m;
                if (A.lp || A.li) {
                    float ent = 0.0f;
                    if (A.lp) ent = A.coef[0] * A.lp[e];
                    if (A.li) ent = A.lp ? fmaf(A.coef[1], A.li[e], ent) : A.coef[1] * A.li[e];
                    t = m - ent;
                }
                A.y[e] = A.done[e] ? rw : fmaf(A.gamma, t, rw);      // a select, as target[done] = rewards_g[done] is
            }
        }
    }
}

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_marl_critic(MarlCriticArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int KS = A.KS, NG = A.NG;
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(2 NG, K3)][2][64]
    const int hsteps = max(2 * NG, K3);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32;

    marl_stage_input(A.state, A.action, A.S, A.NA, A.n_rows, s_in, e0, 0, KS, tid);
    __syncthreads();

    // the net walk of risvec_critic_walk.hpp; called under wave-uniform control flow, ends on a barrier
    auto run_net = [&](const MarlNetPtrs& P, int slot) { marl_run_net<MT2, MT3>(P, slot, s_in, s_h, s_red, L, KS, NG, wave, lane); };
    run_net(A.net[0], 0);
    const bool twin = A.n_nets == 2;                          // a kernel argument: uniform over the grid
    if (twin) run_net(A.net[1], 1);
    marl_epilogue(A, s_red, e0, twin, wave, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_marl_critic_wide: the same launch for inputs that do not fit in LDS beside the activations (16 vehicles: 80 + 288
// inputs = 23 k-steps).  fc1 walks the input in CHUNKS of kWideChunk k-steps: s_in holds one chunk, and a wavefront keeps
// the accumulators of ALL its fc1 groups (at most kWideGroups = 1024 / 32 / 4, 16 registers each) across the chunks.
// Per net and chunk: stage the chunk (zero beyond S + A; rows at or beyond n_rows read row 0), barrier, every wavefront
// runs its groups wave, wave + 4, .. over the chunk's k-steps, barrier before the next chunk overwrites s_in.  Within a
// group the k-steps are added in ascending order into that group's one accumulator, as k_marl_critic adds them: on one
// chunk, and wherever the weights beyond the first chunk are zero, the two kernels give the same bits.  After the last
// chunk bias, ReLU and the split fragments of every group go to s_h; from there on the walk is marl_run_tail and the
// epilogue.  Net 2 stages the input again (s_in held net 1's last chunk).
//
// The accumulators are indexed statically (an unrolled loop over kWideGroups slots under the wave-uniform guard gi <
// ngw): a run-time index would send them to scratch.  The weight prefetch keeps kAhead fragments in flight and walks
// (chunk, group, k-step) in the order the MFMAs do; so that a fragment's register slot is static too, both walk a
// group's k-steps of a chunk in blocks of kAhead positions, and a position beyond the chunk's last k-step neither loads
// nor multiplies.  The prefetch stays on the last position once it has reached it.
constexpr int kWideChunk = 8;        // k-steps of the input that s_in holds
constexpr int kWideGroups = 8;       // fc1 groups a wavefront owns at most: fc1 <= 1024

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_marl_critic_wide(MarlCriticArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5;
    const int KS = A.KS, NG = A.NG;
    uint4* s_in = s_mem;                                      // [kWideChunk][2][64]
    uint4* s_h = s_mem + kWideChunk * 2 * kWave;              // [max(2 NG, K3)][2][64]
    const int hsteps = max(2 * NG, K3);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32;
    const int nch = (KS + kWideChunk - 1) / kWideChunk;       // chunks: a kernel argument's, uniform over the grid
    const int ngw = NG > wave ? (NG - wave + kCriticWaves - 1) / kCriticWaves : 0;      // this wavefront's fc1 groups, <= kWideGroups

    // called under wave-uniform control flow; ends on a barrier
    auto run_net = [&](const MarlNetPtrs& P, int slot) {
        const float u1 = P.scales[0], u2 = P.scales[1], u3 = P.scales[2];
        const uint4* w1 = P.ws + L.fc1 * kWave + lane;
        half8_t ah[kAhead], al[kAhead];
        // (chunk, group slot, position in the group's blocks of kAhead) of the next fetch; fcs k-steps in that chunk
        int fc = 0, fgi = 0, fs = 0, fcs = min(kWideChunk, KS);
        auto fetch = [&](int i) {
            if (fs < fcs) {
                const uint4* p = w1 + (size_t)((wave + kCriticWaves * fgi) * KS + kWideChunk * fc + fs) * (2 * kWave);
                ah[i] = ld_frag(p);
                al[i] = ld_frag(p + kWave);
            }
            if (fs + 1 < ((fcs + kAhead - 1) & -kAhead)) ++fs;
            else if (fgi + 1 < ngw) { ++fgi; fs = 0; }
            else if (fc + 1 < nch) { ++fc; fgi = 0; fs = 0; fcs = min(kWideChunk, KS - kWideChunk * fc); }
            // else: stay on the last position
        };
        f32x16_t d[kWideGroups];
        if (ngw > 0) {                                        // wave-uniform; no barrier inside
#pragma unroll
            for (int i = 0; i < kAhead; ++i) fetch(i);
#pragma unroll
            for (int gi = 0; gi < kWideGroups; ++gi)
#pragma unroll
                for (int q = 0; q < 16; ++q) d[gi][q] = 0.0f;
        }
        for (int c = 0; c < nch; ++c) {
            const int cs = min(kWideChunk, KS - kWideChunk * c);
            if (c > 0) __syncthreads();                       // every wavefront is past the last chunk's MFMAs: s_in is free
            marl_stage_input(A.state, A.action, A.S, A.NA, A.n_rows, s_in, e0, kWideChunk * c, cs, tid);
            __syncthreads();
            if (ngw > 0) {                                    // wave-uniform; no barrier inside
#pragma unroll
                for (int gi = 0; gi < kWideGroups; ++gi) {
                    if (gi < ngw) {
#pragma clang loop unroll(disable)
                        for (int s0 = 0; s0 < cs; s0 += kAhead) {
#pragma unroll
                            for (int i = 0; i < kAhead; ++i) {
                                const int s = s0 + i;
                                if (s < cs) {
                                    const half8_t bh = ld_frag(s_in + (2 * s) * kWave + lane), bl = ld_frag(s_in + (2 * s + 1) * kWave + lane);
                                    d[gi] = mfma3(ah[i], al[i], bh, bl, d[gi]);
                                }
                                fetch(i);
                            }
                        }
                    }
                }
            }
        }
        if (ngw > 0) {
#pragma unroll
            for (int gi = 0; gi < kWideGroups; ++gi) {
                if (gi < ngw) {
                    const int g = wave + kCriticWaves * gi;
                    put_tile(s_h, g, bias_relu(d[gi], u1, tile_of(P.b1, 32 * g, h)), lane);
                }
            }
        }
        __syncthreads();
        marl_run_tail<MT2, MT3>(P, slot, s_h, s_red, L, NG, wave, lane, u2, u3);
    };
    run_net(A.net[0], 0);
    const bool twin = A.n_nets == 2;                          // a kernel argument: uniform over the grid
    if (twin) run_net(A.net[1], 1);
    marl_epilogue(A, s_red, e0, twin, wave, lane);
}

template <int MT2, int MT3>
hipError_t launch_marl(const MarlCriticArgs& a, hipStream_t st) {
    return launch_dynamic_lds(k_marl_critic<MT2, MT3>, dim3((unsigned)((a.n_rows + 31) / 32)), dim3(kMcBlock), marl_walk_lds_bytes(a.KS, a.NG, MT2), st, a);
}

template <int MT2, int MT3>
hipError_t launch_marl_wide(const MarlCriticArgs& a, hipStream_t st) {
    return launch_dynamic_lds(k_marl_critic_wide<MT2, MT3>, dim3((unsigned)((a.n_rows + 31) / 32)), dim3(kMcBlock),
                              marl_walk_lds_bytes(kWideChunk, a.NG, MT2), st, a);
}

// what both kernels take; a shape either rule covers
MarlCriticArgs marl_args(long long n_rows, int S, int A, int F1, int n_nets, const RisVecMarlCriticNet* nets, const float* state,
                         const float* action, const float* reward, const uint8_t* done, float gamma, const float* coef,
                         const float* logp_power, const float* logp_intent, float* q1, float* q2, float* y) {
    MarlCriticArgs c{};
    c.n_rows = n_rows; c.S = S; c.NA = A; c.KS = ks_of(S + A); c.NG = F1 / 32; c.n_nets = n_nets;
    c.state = state; c.action = action;
    for (int i = 0; i < 2; ++i) c.net[i] = marl_net_ptrs(nets[i < n_nets ? i : 0]);      // a single net fills both slots
    c.reward = reward; c.done = done; c.gamma = gamma; c.coef = coef; c.lp = logp_power; c.li = logp_intent;
    c.q1 = q1; c.q2 = q2; c.y = y;
    return c;
}

bool fc_supported(int F1, int F2, int F3) {
    return F1 >= 32 && F1 % 32 == 0 && F1 <= 1024 && (F2 == 128 || F2 == 256 || F2 == 512) && (F3 == 128 || F3 == 256);
}

}  // namespace

bool marl_critic_supported(int S, int A, int F1, int F2, int F3) {
    return S >= 1 && A >= 1 && S <= 127 && A <= 127 && S + A <= 128 && fc_supported(F1, F2, F3);
}

// Deliberately overlaps the rule above: on a shape both cover, the two kernels are compared bit for bit.  fc1 <= 1024
// is kWideGroups groups per wavefront.
bool marl_critic_wide_supported(int S, int A, int F1, int F2, int F3) {
    static_assert(kWideGroups * kCriticWaves * 32 == 1024, "a wavefront holds the accumulators of all its fc1 groups");
    return S >= 1 && A >= 1 && S <= 511 && A <= 511 && S + A <= 512 && fc_supported(F1, F2, F3);
}

long long marl_critic_stream_bytes(int S, int A, int F1, int F2, int F3) {
    if (!marl_critic_supported(S, A, F1, F2, F3)) return 0;
    return marl_layout(ks_of(S + A), F1 / 32, F2 / 128, F3 / 128).rows * kWave * (long long)sizeof(uint4);
}

long long marl_critic_wide_stream_bytes(int S, int A, int F1, int F2, int F3) {
    if (!marl_critic_wide_supported(S, A, F1, F2, F3)) return 0;
    return marl_layout(ks_of(S + A), F1 / 32, F2 / 128, F3 / 128).rows * kWave * (long long)sizeof(uint4);
}

hipError_t launch_marl_critic(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticNet* nets,
                              const float* state, const float* action, const float* reward, const uint8_t* done, float gamma,
                              const float* coef, const float* logp_power, const float* logp_intent, float* q1, float* q2,
                              float* y, hipStream_t st) {
    if (!marl_critic_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2) return hipErrorInvalidValue;
    const MarlCriticArgs c = marl_args(n_rows, S, A, F1, n_nets, nets, state, action, reward, done, gamma, coef, logp_power,
                                       logp_intent, q1, q2, y);
    note_kernel("k_marl_critic<%d,%d>x%d", F2 / 128, F3 / 128, n_nets);
    return dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) { return launch_marl<decltype(mt2)::value, decltype(mt3)::value>(c, st); });
}

hipError_t launch_marl_critic_wide(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets,
                                   const RisVecMarlCriticNet* nets, const float* state, const float* action, const float* reward,
                                   const uint8_t* done, float gamma, const float* coef, const float* logp_power,
                                   const float* logp_intent, float* q1, float* q2, float* y, hipStream_t st) {
    if (!marl_critic_wide_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2) return hipErrorInvalidValue;
    const MarlCriticArgs c = marl_args(n_rows, S, A, F1, n_nets, nets, state, action, reward, done, gamma, coef, logp_power,
                                       logp_intent, q1, q2, y);
    note_kernel("k_marl_critic_wide<%d,%d>x%d", F2 / 128, F3 / 128, n_nets);
    return dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) { return launch_marl_wide<decltype(mt2)::value, decltype(mt3)::value>(c, st); });
}

}  // namespace risvec
