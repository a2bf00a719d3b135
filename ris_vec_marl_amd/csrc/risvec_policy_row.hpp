// The row math of the reference's `PolicyNetwork.sample_normal` (sac_agent.py, SAC below) that the batched
// choose_action (k_policy.hip::k_policy_sample) and the learner's sample_normal (k_policy_learn.hip) share, so that
// for the same heads and draws both kernels produce the same bits: the Gumbel-softmax of the masked logits with its
// arg-max (SAC:91-113) and the tanh-squashed Normal sample (SAC:72, 83-86).  VP = pow2ceil(V) lanes per (row, agent),
// lane k owns logit k; max / arg-max / sum over a row are log2(VP) DPP exchanges.
#pragma once
#include <cfloat>

#include "risvec_dev.hpp"
#include "risvec_step.hpp"      // DPP exchanges (xchg / gsum)

namespace risvec {

constexpr uint32_t kSitePolicyEps = 9, kSitePolicyGumbel = 10;

struct PolicyIntent {
    float pk;       // y_k: soft Gumbel-softmax, or its straight-through form where hard[v]
    int arg;        // arg-max of the row, first index on ties
    float ml;       // this lane's masked logit (SAC:91-106); -inf on the lanes k >= V
};

// h: the (row, agent) head row (mu[2], log_std[2], logits[V]); gid = row * V + v indexes mask / expo [rows, V, V];
// genv: the Philox key of the row (offset + row).  Every lane of the VP-lane group must call it.
template <int VP>
__device__ __forceinline__ PolicyIntent policy_row_intent(const float* h, const uint8_t* mask, const float* expo, const float* tau,
                                                          const uint8_t* hard, long long gid, int V, int v, int k, uint32_t genv,
                                                          uint32_t counter, uint64_t seed) {
    const bool open_k = k < V && (!mask || mask[gid * V + k] != 0);
    const bool any_open = gsum<VP>(mask && open_k ? 1.0f : 0.0f) > 0.0f;
    const bool blocked = mask && any_open && !open_k;          // an all-zero row is opened up (SAC:97-100)
    float z = -INFINITY, ml = -INFINITY;
    if (k < V) {
        float ex;
        if (expo) ex = expo[gid * V + k];
        else {
            const uint4 r = philox4x32_10(genv, (uint32_t)v, counter, kSitePolicyGumbel + 0x100u * (k >> 2), seed);
            const uint32_t x = (k & 3) == 0 ? r.x : (k & 3) == 1 ? r.y : (k & 3) == 2 ? r.z : r.w;
            // Exp(1), u in (0, 1].  u == 1 would be 0, its Gumbel +inf and the row inf - inf: as torch's device
            // exponential_() does (what F.gumbel_softmax draws with, SAC:110-113), that one draw is 2^-24 instead
            const uint32_t m = x >> 8;
            ex = m == 0xFFFFFFu ? 0x1p-24f : -logf(((float)m + 1.0f) * 0x1p-24f);
        }
        ml = blocked ? -FLT_MAX / 2.0f : h[4 + k];                    // torch.finfo(float32).min / 2  (SAC:103)
        z = (ml + -logf(ex)) / tau[v];                                // (logits + gumbel) / tau
    }
    float zmax = z;
    int arg = k < V ? k : 0x7fffffff;
#pragma unroll
    for (int o = 1; o < VP; o <<= 1) {                                // arg-max, first index on ties
        float oz; int oa;
        if (o == 1) { oz = xchg<1>(zmax); oa = __builtin_bit_cast(int, xchg<1>(__builtin_bit_cast(float, arg))); }
        else if (o == 2) { oz = xchg<2>(zmax); oa = __builtin_bit_cast(int, xchg<2>(__builtin_bit_cast(float, arg))); }
        else if (o == 4) { oz = xchg<4>(zmax); oa = __builtin_bit_cast(int, xchg<4>(__builtin_bit_cast(float, arg))); }
        else if (o == 8) { oz = xchg<8>(zmax); oa = __builtin_bit_cast(int, xchg<8>(__builtin_bit_cast(float, arg))); }
        else if (o == 16) { oz = xchg<16>(zmax); oa = __builtin_bit_cast(int, xchg<16>(__builtin_bit_cast(float, arg))); }
        else { oz = xchg<32>(zmax); oa = __builtin_bit_cast(int, xchg<32>(__builtin_bit_cast(float, arg))); }
        if (oz > zmax || (oz == zmax && oa < arg)) { zmax = oz; arg = oa; }
    }
    const float ez = k < V ? expf(z - zmax) : 0.0f;
    const float sum = gsum<VP>(ez);
    float pk = ez / sum;
    if (hard && hard[v]) pk = ((k == arg ? 1.0f : 0.0f) - pk) + pk;   // y_hard - y_soft + y_soft (SAC:110-113)
    return PolicyIntent{pk, arg, ml};
}

struct PolicyPower {
    float e0, e1;       // the N(0,1) draws
    float ls0, ls1;     // clamped log_std (SAC:72)
    float p0, p1;       // tanh(mu + std eps) (SAC:83-86)
};

// eps [rows, V, 2] or NULL (Philox).  One lane per (row, agent) calls it.
__device__ __forceinline__ PolicyPower policy_row_power(const float* h, const float* eps, long long gid, int v, uint32_t genv,
                                                        uint32_t counter, uint64_t seed) {
    float e0, e1;
    if (eps) { e0 = eps[gid * 2]; e1 = eps[gid * 2 + 1]; }
    else {
        const uint4 r = philox4x32_10(genv, (uint32_t)v, counter, kSitePolicyEps, seed);
        const float2 n = normal2(r.x, r.y);
        e0 = n.x; e1 = n.y;
    }
    const float ls0 = fminf(fmaxf(h[2], -20.0f), 2.0f), ls1 = fminf(fmaxf(h[3], -20.0f), 2.0f);
    const float p0 = tanhf(e0 * expf(ls0) + h[0]), p1 = tanhf(e1 * expf(ls1) + h[1]);
    return PolicyPower{e0, e1, ls0, ls1, p0, p1};
}

}  // namespace risvec
