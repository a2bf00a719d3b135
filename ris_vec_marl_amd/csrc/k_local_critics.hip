// Every agent's local twin target critics and local TD target of the multi-agent (SAC) learner -- Agent.local_learn,
// Simulation-MARL-BCD/sac_agent.py:263-284, called once per agent by global_sac_critic.py:373-392 -- in ONE kernel for
// n_rows rows and n_agents agents.  Grid (ceil(n_rows / 32), n_agents): workgroup (tile, j) does for agent j exactly what a
// k_marl_critic workgroup does for the global critic (read that file's header) -- the same net walk, instantiated from
// risvec_critic_walk.hpp -- with agent j's two weight streams, biases and q layers, on agent j's columns of the batch:
//     x   = [obs[row, j, 0:S] | action_j | 0 ..]
//     action_j = action[row, j, 0:A]                                           explicit form
//              = [onehot(idx) (n_agents) | power[row, j, 0:2]]                 from the policy (A == n_agents + 2)
//         idx  = the first maximum of heads[j, row, 4 + i], i < n_agents, entry i == j REPLACED by finfo(float32).min / 2
//                (sac_agent.py:270-272: replaced, not excluded, so it still wins where every other logit is lower still)
//     m   = n_nets == 2 ? min(q_1, q_2) : q_1
//     t   = m - (coef[0] lp[row, j] + coef[1] li[row, j])                      a term whose logp pointer is NULL is absent
//     y[j, row] = reward[row, j] + ((1 - done[row]) gamma) t                   a PRODUCT, as :284 is: a done row with an
//                                                                              infinite t gives NaN, as the reference does
// Every float operation of the epilogue is rounded on its own (no fused multiply-add), as the reference's statements are.
// The per-agent input never exists in memory.  A NaN logit is not supported (torch.argmax would pick it).
//
// Every barrier sits under wave-uniform control flow: loop bounds and the net count come from kernel arguments, template
// parameters and the wavefront index; the agent is blockIdx.y.  Rows at or beyond n_rows are computed on row 0's input
// and never stored.  No global address depends on loaded data -- idx decides a VALUE of the staged input, never an
// address -- and every weight prefetch index is clamped to the last fragment of its block.
#include "risvec_critic_walk.hpp"
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"
#include "risvec_step.hpp"

namespace risvec {
namespace {

struct LocalCriticsArgs {
    long long n_rows;
    int V, S, NA, KS, NG, n_nets;  // V agents; KS = k-steps of 16 of [obs_j | action_j]; NG = fc1 / 32
    float gamma;
    const float* obs;              // [n_rows, V, S]
    const float* action;           // [n_rows, V, NA] or NULL
    const float* heads;            // [V, n_rows, 4 + V] or NULL (then action)
    const float* power;            // [n_rows, V, 2], with heads
    const float* reward;           // [n_rows, V] or NULL
    const uint8_t* done;           // [n_rows] or NULL
    const float* coef;             // [2] or NULL
    const float* lp;               // [n_rows, V] or NULL
    const float* li;               // [n_rows, V] or NULL
    float* q1;                     // [V, n_rows] or NULL
    float* q2;                     // [V, n_rows] or NULL
    float* y;                      // [V, n_rows] or NULL
    MarlNetPtrs net[kLocalCriticsMaxAgents * 2];              // agent j's net c at [j n_nets + c]
};

constexpr float kSelfLogit = -3.40282346638528859812e38f / 2;        // finfo(float32).min / 2

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_local_critics(LocalCriticsArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int KS = A.KS, NG = A.NG, V = A.V;
    const int agent = blockIdx.y;                             // uniform over the workgroup
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(2 NG, K3)][2][64]
    const int hsteps = max(2 * NG, K3);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32;

    // ---- the input as split B fragments: k-step s, lane (r, h) holds x[16 s + 8 h + j], j < 8; x = [obs_j | action_j | 0 ..]
    {
        const int S = A.S, NA = A.NA, W = S + NA;
        const bool from_policy = A.heads != nullptr;          // a kernel argument: uniform over the grid
        for (int idx = tid; idx < KS * kWave; idx += kMcBlock) {
            const int s = idx >> 6, l = idx & 63, rr = l & 31, hh = l >> 5;
            const long long row = e0 + rr < A.n_rows ? e0 + rr : 0;
            const float* ps = A.obs + (row * V + agent) * S;
            const int k0 = 16 * s + 8 * hh;
            f32x8_t v;
            if (!from_policy) {
                const float* pa = A.action + (row * V + agent) * NA;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + j;
                    v[j] = k < S ? ps[k] : (k < W ? pa[k - S] : 0.0f);
                }
            } else {
                int pick = 0;
                if (k0 + 8 > S && k0 < S + V) {               // these 8 values meet the one-hot
                    const float* lg = A.heads + ((long long)agent * A.n_rows + row) * (4 + V) + 4;
                    float best = agent == 0 ? kSelfLogit : lg[0];
                    for (int i = 1; i < V; ++i) {
                        const float x = i == agent ? kSelfLogit : lg[i];
                        if (x > best) { best = x; pick = i; }  // strictly greater: the lowest index wins a tie
                    }
                }
                const float* pp = A.power + (row * V + agent) * 2;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + j;
                    v[j] = k < S ? ps[k] : (k < S + V ? (k - S == pick ? 1.0f : 0.0f) : (k < W ? pp[k - S - V] : 0.0f));
                }
            }
            put_input(s_in, s, l, v);
        }
    }
    __syncthreads();

    const bool twin = A.n_nets == 2;                          // a kernel argument: uniform over the grid
    const MarlNetPtrs P1 = A.net[agent * A.n_nets];
    marl_run_net<MT2, MT3>(P1, 0, s_in, s_h, s_red, L, KS, NG, wave, lane);
    const MarlNetPtrs P2 = A.net[agent * A.n_nets + (twin ? 1 : 0)];
    if (twin) marl_run_net<MT2, MT3>(P2, 1, s_in, s_h, s_red, L, KS, NG, wave, lane);

    if (wave == 0 && h == 0) {
        const long long e = e0 + r;
        if (e < A.n_rows) {
            const long long o = (long long)agent * A.n_rows + e, i = e * V + agent;
            const float qv1 = marl_red(s_red, 0, r) + P1.qb[0];
            float m = qv1;
            if (A.q1) A.q1[o] = qv1;
            if (twin) {
                const float qv2 = marl_red(s_red, 1, r) + P2.qb[0];
                if (A.q2) A.q2[o] = qv2;
                m = fminf(qv1, qv2);
            }
            if (A.y) {
#pragma clang fp contract(off)                                // every operation rounded on its own, as the reference's statements
                float t = m;
                if (A.lp && A.li) t = m - (A.coef[0] * A.lp[i] + A.coef[1] * A.li[i]);
                else if (A.lp) t = m - A.coef[0] * A.lp[i];
                else if (A.li) t = m - A.coef[1] * A.li[i];
                const float live = (A.done[e] ? 0.0f : 1.0f) * A.gamma;
                A.y[o] = A.reward[i] + live * t;              // a product, not a select (sac_agent.py:284)
            }
        }
    }
}

template <int MT2, int MT3>
hipError_t launch_local(const LocalCriticsArgs& a, hipStream_t st) {
    return launch_dynamic_lds(k_local_critics<MT2, MT3>, dim3((unsigned)((a.n_rows + 31) / 32), (unsigned)a.V), dim3(kMcBlock),
                              marl_walk_lds_bytes(a.KS, a.NG, MT2), st, a);
}

}  // namespace

bool local_critics_supported(int V, int S, int A, int F1, int F2, int F3) {
    return V >= 1 && V <= kLocalCriticsMaxAgents && marl_critic_supported(S, A, F1, F2, F3);
}

hipError_t launch_local_critics(long long n_rows, int V, int S, int A, int F1, int F2, int F3, int n_nets,
                                const RisVecMarlCriticNet* nets, const float* obs, const float* action, const float* heads,
                                const float* power, const float* reward, const uint8_t* done, float gamma, const float* coef,
                                const float* logp_power, const float* logp_intent, float* q1, float* q2, float* y, hipStream_t st) {
    if (!local_critics_supported(V, S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2) return hipErrorInvalidValue;
    if (heads && A != V + 2) return hipErrorInvalidValue;
    LocalCriticsArgs c{};
    c.n_rows = n_rows; c.V = V; c.S = S; c.NA = A; c.KS = ks_of(S + A); c.NG = F1 / 32; c.n_nets = n_nets; c.gamma = gamma;
    c.obs = obs; c.action = action; c.heads = heads; c.power = power;
    for (int i = 0; i < kLocalCriticsMaxAgents * 2; ++i)
        c.net[i] = marl_net_ptrs(nets[i < V * n_nets ? i : 0]);   // the unused slots repeat the first net
    c.reward = reward; c.done = done; c.coef = coef; c.lp = logp_power; c.li = logp_intent;
    c.q1 = q1; c.q2 = q2; c.y = y;
    note_kernel("k_local_critics<%d,%d>x%dx%d", F2 / 128, F3 / 128, V, n_nets);
    return dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) { return launch_local<decltype(mt2)::value, decltype(mt3)::value>(c, st); });
}

}  // namespace risvec
