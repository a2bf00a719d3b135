// The learner's `policy.sample_normal(obs_j, mask=mask_j)` (sac_agent.py:80-127, SAC below) for every sampled row and
// every agent in one launch, with what `global_learn` (global_sac_critic.py:326-336, GSC below) does with its results:
// the next_actions row of the target critics (per agent the arg-max one-hot, then the powers) and the log-probability
// sums over the agents.  Input: the heads [V, B, 4+V] of the policy forward (risvec_policy_mlp / risvec_policy_heads).
//
// The sample itself -- log_std clamp, x_t = mu + std eps, tanh, masked logits, Gumbel-softmax, arg-max -- is the row
// math of risvec_policy_row.hpp, shared with k_policy_sample: same heads and draws, same bits.  On top of it, in float32:
//
//   logp_power[b,v]  = sum_{i<2} ( -eps_i^2 / 2 - log_std_i - log(2 pi) / 2 - log(1 - p_i^2 + 1e-6) )           (SAC:87-88)
//     The Normal term uses the draw `eps` itself, not ((x_t - mu)^2) / (2 var) as the reference's float32 tensors do:
//     the two are equal in exact arithmetic, but x_t - mu cancels when std is small (at log_std = -20 every digit of
//     eps is gone), and the eps form is the one a float64 evaluation of the reference's formula agrees with.
//   logp_intent[b,v] = sum_k y_k lsm_k (soft)  or  lsm[argmax y] (hard[v]),  lsm = log_softmax(masked logits): row max
//     subtracted, logsumexp over the row, no temperature, no Gumbel (SAC:116-124).  A blocked entry is
//     finfo(float32).min / 2: its y is exactly 0 (also when tau < 0.5 takes the divided logit to -inf) and its lsm is
//     finite, so 0 * lsm stays 0; the product is skipped where y == 0 all the same.
//
// Layout: VP = pow2ceil(V) lanes per (row, agent) slot, kBlock / VP slots per workgroup.  For V <= 16 (V VP <= kBlock)
// a workgroup owns n = (kBlock / VP) / V whole batch rows: slot s is (row s / V, agent s % V), slots past n V are dead.
// Lane 0 of a slot leaves the two log-probabilities in LDS, and after a barrier one lane per batch row adds them in agent
// order 0 .. V-1 (as the loop GSC:335-336 does): deterministic, no atomics.  For V > 16 the slots are the flat
// (row, agent) list and there are no sums (the entry point refuses the pointers).  Dead slots shadow the last live row
// and store nothing.
#include "risvec_launch.hpp"
#include "risvec_policy_row.hpp"

namespace risvec {
namespace {

struct PolicyLearnArgs {
    int B, V;
    long long row_offset;
    const float* heads;        // [V, B, 4 + V]
    const uint8_t* mask;       // [B, V, V] or NULL
    const float* tau;          // [V]
    const uint8_t* hard;       // [V] or NULL
    const float* eps;          // [B, V, 2] or NULL
    const float* expo;         // [B, V, V] or NULL
    uint64_t seed;
    uint32_t counter;
    float* power;              // [B, V, 2] or NULL
    float* probs;              // [B, V, V] or NULL
    float* next_actions;       // [B, V, V + 2] or NULL
    float* logp_power;         // [B, V] or NULL
    float* logp_intent;        // [B, V] or NULL
    float* logp_power_sum;     // [B] or NULL (V <= 16)
    float* logp_intent_sum;    // [B] or NULL (V <= 16)
};

constexpr float kHalfLog2Pi = 0.91893853320467274f;

template <int VP>
__device__ __forceinline__ float gmax(float x) {
    if constexpr (VP >= 64) x = fmaxf(x, xchg<32>(x));
    if constexpr (VP >= 32) x = fmaxf(x, xchg<16>(x));
    if constexpr (VP >= 16) x = fmaxf(x, xchg<8>(x));
    if constexpr (VP >= 8) x = fmaxf(x, xchg<4>(x));
    if constexpr (VP >= 4) x = fmaxf(x, xchg<2>(x));
    if constexpr (VP >= 2) x = fmaxf(x, xchg<1>(x));
    return x;
}

template <int VP>
__global__ void __launch_bounds__(kBlock)
k_policy_sample_normal(PolicyLearnArgs A) {
    constexpr int S = kBlock / VP;                             // (row, agent) slots per workgroup
    __shared__ float s_lp[2][S];
    const int V = A.V, H = 4 + V;
    const int n = S / V;                                       // batch rows a workgroup owns; 0: flat slots (V > 16)
    const int s = threadIdx.x / VP, k = threadIdx.x % VP;
    const long long n_rows = (long long)A.B * V;
    long long row_raw;
    bool live_row;
    if (n > 0) {
        const long long b_own = (long long)blockIdx.x * n + s / V;
        live_row = s < n * V && b_own < A.B;
        row_raw = b_own * V + s % V;
    } else {
        row_raw = (long long)blockIdx.x * S + s;
        live_row = row_raw < n_rows;
    }
    const long long gid = live_row ? row_raw : n_rows - 1;     // dead slots shadow the last row, store nothing
    const bool mine = live_row && k < V;
    const long long b = gid / V;
    const int v = (int)(gid % V);
    const float* h = A.heads + ((long long)v * A.B + b) * H;
    const uint32_t genv = (uint32_t)(A.row_offset + b);
    // ---- discrete head: y, arg-max (shared row math), then log_softmax of the masked logits  (SAC:91-124) ----------
    const PolicyIntent I = policy_row_intent<VP>(h, A.mask, A.expo, A.tau, A.hard, gid, V, v, k, genv, A.counter, A.seed);
    const float d = I.ml - gmax<VP>(I.ml);                     // lanes k >= V hold -inf and stay out of max and sum
    const float lse = logf(gsum<VP>(k < V ? expf(d) : 0.0f));
    const float lsm = d - lse;
    float term;
    if (A.hard && A.hard[v]) term = k == I.arg ? lsm : 0.0f;
    else term = (k < V && I.pk != 0.0f) ? I.pk * lsm : 0.0f;
    const float lp_int = gsum<VP>(term);
    if (mine) {
        if (A.probs) A.probs[gid * V + k] = I.pk;
        if (A.next_actions) A.next_actions[gid * (V + 2) + k] = k == I.arg ? 1.0f : 0.0f;     // GSC:328-332
    }
    // ---- continuous head, lane 0 of the slot  (SAC:72, 83-88) ------------------------------------------------------
    if (live_row && k == 0) {
        const PolicyPower P = policy_row_power(h, A.eps, gid, v, genv, A.counter, A.seed);
        const float t0 = -0.5f * P.e0 * P.e0 - P.ls0 - kHalfLog2Pi - logf(1.0f - P.p0 * P.p0 + 1e-6f);
        const float t1 = -0.5f * P.e1 * P.e1 - P.ls1 - kHalfLog2Pi - logf(1.0f - P.p1 * P.p1 + 1e-6f);
        const float lp_pow = t0 + t1;
        if (A.power) { A.power[gid * 2] = P.p0; A.power[gid * 2 + 1] = P.p1; }
        if (A.next_actions) {                                                                 // GSC:333
            A.next_actions[gid * (V + 2) + V] = P.p0;
            A.next_actions[gid * (V + 2) + V + 1] = P.p1;
        }
        if (A.logp_power) A.logp_power[gid] = lp_pow;
        if (A.logp_intent) A.logp_intent[gid] = lp_int;
        s_lp[0][s] = lp_pow;
        s_lp[1][s] = lp_int;
    }
    // ---- sums over the agents, in agent order  (GSC:335-336) -------------------------------------------------------
    if (n > 0 && (A.logp_power_sum || A.logp_intent_sum)) {    // uniform over the grid: every lane meets the barrier
        __syncthreads();
        const long long b_sum = (long long)blockIdx.x * n + threadIdx.x;
        if ((int)threadIdx.x < n && b_sum < A.B) {             // the row is live, so its V slots were all written
            float sp = 0.0f, si = 0.0f;
            for (int a = 0; a < V; ++a) {
                sp += s_lp[0][threadIdx.x * V + a];
                si += s_lp[1][threadIdx.x * V + a];
            }
            if (A.logp_power_sum) A.logp_power_sum[b_sum] = sp;
            if (A.logp_intent_sum) A.logp_intent_sum[b_sum] = si;
        }
    }
}

}  // namespace

int policy_sample_normal_rows_per_block(int V) {
    const int vp = pow2_ceil(V);
    return (kBlock / vp) / V;
}

hipError_t launch_policy_sample_normal(int B, int V, long long row_offset, const float* heads, const uint8_t* mask,
                                       const float* tau, const uint8_t* hard, const float* eps, const float* expo,
                                       uint64_t seed, uint32_t counter, float* power, float* probs, float* next_actions,
                                       float* logp_power, float* logp_intent, float* logp_power_sum, float* logp_intent_sum,
                                       hipStream_t st) {
    PolicyLearnArgs a{B, V, row_offset, heads, mask, tau, hard, eps, expo, seed, counter, power, probs, next_actions,
                      logp_power, logp_intent, logp_power_sum, logp_intent_sum};
    const int vp = pow2_ceil(V), n = policy_sample_normal_rows_per_block(V);
    if (n == 0 && (logp_power_sum || logp_intent_sum)) return hipErrorInvalidValue;
    const long long blocks = n > 0 ? ((long long)B + n - 1) / n : ((long long)B * V * vp + kBlock - 1) / kBlock;
    if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    switch (vp) {
        case 1: hipLaunchKernelGGL(k_policy_sample_normal<1>, grid, dim3(kBlock), 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_policy_sample_normal<2>, grid, dim3(kBlock), 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_policy_sample_normal<4>, grid, dim3(kBlock), 0, st, a); break;
        case 8: hipLaunchKernelGGL(k_policy_sample_normal<8>, grid, dim3(kBlock), 0, st, a); break;
        case 16: hipLaunchKernelGGL(k_policy_sample_normal<16>, grid, dim3(kBlock), 0, st, a); break;
        case 32: hipLaunchKernelGGL(k_policy_sample_normal<32>, grid, dim3(kBlock), 0, st, a); break;
        default: hipLaunchKernelGGL(k_policy_sample_normal<64>, grid, dim3(kBlock), 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace risvec
