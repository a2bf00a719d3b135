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
// The net walk (the fc1 group walk, fc2, fc3, the q dot product, the s_red reduction) and the input-fragment store are
// risvec_critic_walk.hpp's, instantiated here and by k_local_critics.hip.
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

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_marl_critic(MarlCriticArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int KS = A.KS, NG = A.NG;
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(2 NG, K3)][2][64]
    const int hsteps = max(2 * NG, K3);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32;

    // ---- the input as split B fragments: k-step s, lane (r, h) holds x[16 s + 8 h + j], j < 8; x = [state | action | 0 ..]
    {
        const int S = A.S, W = A.S + A.NA;
        for (int idx = tid; idx < KS * kWave; idx += kMcBlock) {
            const int s = idx >> 6, l = idx & 63, rr = l & 31, hh = l >> 5;
            const long long row = e0 + rr < A.n_rows ? e0 + rr : 0;
            const float* ps = A.state + row * S;
            const float* pa = A.action + row * A.NA;
            f32x8_t v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * hh + j;
                v[j] = k < S ? ps[k] : (k < W ? pa[k - S] : 0.0f);
            }
            put_input(s_in, s, l, v);
        }
    }
    __syncthreads();

    // the net walk of risvec_critic_walk.hpp; called under wave-uniform control flow, ends on a barrier
    auto run_net = [&](const MarlNetPtrs& P, int slot) { marl_run_net<MT2, MT3>(P, slot, s_in, s_h, s_red, L, KS, NG, wave, lane); };
    run_net(A.net[0], 0);
    const bool twin = A.n_nets == 2;                          // a kernel argument: uniform over the grid
    if (twin) run_net(A.net[1], 1);

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
hipError_t launch_marl(const MarlCriticArgs& a, hipStream_t st) {
    return launch_dynamic_lds(k_marl_critic<MT2, MT3>, dim3((unsigned)((a.n_rows + 31) / 32)), dim3(kMcBlock), marl_walk_lds_bytes(a.KS, a.NG, MT2), st, a);
}

}  // namespace

bool marl_critic_supported(int S, int A, int F1, int F2, int F3) {
    return S >= 1 && A >= 1 && S <= 127 && A <= 127 && S + A <= 128 && F1 >= 32 && F1 % 32 == 0 && F1 <= 1024 &&
           (F2 == 128 || F2 == 256 || F2 == 512) && (F3 == 128 || F3 == 256);
}

long long marl_critic_stream_bytes(int S, int A, int F1, int F2, int F3) {
    if (!marl_critic_supported(S, A, F1, F2, F3)) return 0;
    return marl_layout(ks_of(S + A), F1 / 32, F2 / 128, F3 / 128).rows * kWave * (long long)sizeof(uint4);
}

hipError_t launch_marl_critic(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticNet* nets,
                              const float* state, const float* action, const float* reward, const uint8_t* done, float gamma,
                              const float* coef, const float* logp_power, const float* logp_intent, float* q1, float* q2,
                              float* y, hipStream_t st) {
    if (!marl_critic_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2) return hipErrorInvalidValue;
    MarlCriticArgs c{};
    c.n_rows = n_rows; c.S = S; c.NA = A; c.KS = ks_of(S + A); c.NG = F1 / 32; c.n_nets = n_nets;
    c.state = state; c.action = action;
    for (int i = 0; i < 2; ++i) c.net[i] = marl_net_ptrs(nets[i < n_nets ? i : 0]);      // a single net fills both slots
    c.reward = reward; c.done = done; c.gamma = gamma; c.coef = coef; c.lp = logp_power; c.li = logp_intent;
    c.q1 = q1; c.q2 = q2; c.y = y;
    note_kernel("k_marl_critic<%d,%d>x%d", F2 / 128, F3 / 128, n_nets);
    return dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) { return launch_marl<decltype(mt2)::value, decltype(mt3)::value>(c, st); });
}

}  // namespace risvec
