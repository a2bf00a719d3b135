// Internal launcher declarations (one per kernel family); argument validation lives
// in risvec_api.hip, these only compute the grid and launch.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "risvec.h"
#include "risvec_dev.hpp"

namespace risvec {

hipError_t launch_reset(const RisVecState& s, const RisVecParams& p, const int32_t* spawn_ints,
                        const int32_t* buf0, uint64_t seed, uint32_t counter, hipStream_t st);
hipError_t launch_mobility(const RisVecState& s, const RisVecParams& p, const float* u_turn,
                           int32_t* n_used, uint64_t seed, uint32_t counter, hipStream_t st);
hipError_t launch_geometry(const RisVecState& s, const RisVecParams& p, hipStream_t st);
hipError_t launch_gain_3gpp(const RisVecState& s, const RisVecParams& p, int32_t model,
                            const float* u_los, const float* z_shadow, const float* small,
                            uint64_t seed, uint32_t counter, hipStream_t st);
hipError_t launch_set_phase(const RisVecState& s, const float* angle, hipStream_t st);
hipError_t launch_random_phase(const RisVecState& s, const int32_t* idx, uint64_t seed,
                               uint32_t counter, hipStream_t st);

hipError_t launch_gain(const RisVecState& s, const RisVecParams& p, hipStream_t st);
struct StepRing;
hipError_t launch_step(const RisVecState& s, const RisVecParams& p, const float* action,
                       const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals,
                       uint64_t seed, uint32_t counter, uint32_t flags, bool fused, hipStream_t st,
                       const StepRing* ring = nullptr);

hipError_t launch_data_rate(const RisVecState& s, const RisVecParams& p, const float* p_off,
                            const int32_t* partner, const int32_t* n_groups, float* rate_out,
                            hipStream_t st);

hipError_t launch_colsum(const RisVecState& s, hipStream_t st);
hipError_t launch_bcd(const RisVecState& s, const RisVecParams& p, int32_t* idx_out, bool reuse_colsum,
                      bool reuse_s, bool reuse_idx, bool write_theta, hipStream_t st);
hipError_t launch_step_fused_bcd(const RisVecState& s, const RisVecParams& p, const float* action,
                                 const int32_t* partner, const int32_t* n_groups,
                                 const int32_t* arrivals, uint64_t seed, uint32_t counter,
                                 uint32_t flags, hipStream_t st);

hipError_t launch_sarl_step(const RisVecState& s, const RisVecSarlParams& p, const float* action_power,
                            const float* action_phase, const int32_t* arrivals, uint64_t seed,
                            uint32_t counter, uint32_t flags, hipStream_t st);

long long noma_scratch_bytes(int n_envs, int n_veh);
hipError_t launch_noma_begin_episode(const RisVecNomaState& ns, hipStream_t st);
hipError_t launch_noma_mask(const RisVecNomaState& ns, const float* gain, const double* gdb15, double q_now,
                            int K_now, hipStream_t st);
hipError_t launch_noma_group(const RisVecNomaState& ns, const RisVecNomaParams& p, const float* gain,
                             const double* gdb12, const float* p01, int p01_raw, int use_mask, int K_back,
                             const double* tau_back, const float* prev_global, int prev_stride, int i_step,
                             const float* u_unstick, uint64_t seed, uint32_t counter, int32_t* info_out,
                             hipStream_t st);
hipError_t launch_noma_flush(const RisVecNomaState& ns, float decay, hipStream_t st);

hipError_t launch_replay_store(const RisVecReplay& rb, long long cursor, int n, const float* state, const float* action,
                               const float* power_raw, const float* probs, const float* reward_g, int rg_stride, const float* reward_l, const float* state_,
                               const uint8_t* done, int done_all, const uint8_t* mask, float* carry, hipStream_t st);
hipError_t launch_replay_sample(const RisVecReplay& rb, long long max_mem, int batch, const int64_t* idx, uint64_t seed,
                                uint32_t counter, float* states, float* actions, float* rewards_g, float* rewards_l,
                                float* states_, uint8_t* dones, float* masks, int64_t* idx_out, hipStream_t st);
hipError_t launch_marshal_actions(int E, int V, const float* power_raw, const float* probs, float floor_eff,
                                  float* action_env, float* p_off01, float* action_store, hipStream_t st);

hipError_t launch_policy_sample(int E, int V, long long env_offset, const float* heads, const uint8_t* mask,
                                const float* tau, const uint8_t* hard, const float* eps, const float* expo, uint64_t seed,
                                uint32_t counter, float floor_eff, float* power_raw, float* probs, float* onehot,
                                float* action_env, float* p_off01, float* action_store, hipStream_t st);

// sample_normal of every (row, agent) with the learner's next_actions and log-prob sums (k_policy_learn.hip).
// policy_sample_normal_rows_per_block(): batch rows one workgroup owns (0 for V > 16: no sums).
int policy_sample_normal_rows_per_block(int V);
hipError_t launch_policy_sample_normal(int B, int V, long long row_offset, const float* heads, const uint8_t* mask,
                                       const float* tau, const uint8_t* hard, const float* eps, const float* expo,
                                       uint64_t seed, uint32_t counter, float* power, float* probs, float* next_actions,
                                       float* logp_power, float* logp_intent, float* logp_power_sum, float* logp_intent_sum,
                                       hipStream_t st);

hipError_t launch_policy_layer1(int E, int V, int IN, int F, const float* obs, const float* W1, const float* b1,
                                const float* lw, const float* lb, float* out, hipStream_t st);
hipError_t launch_policy_layer1_split16(int E, int V, int IN, int F, const float* obs, const float* W1, const float* b1,
                                        const float* lw, const float* lb, void* out16, hipStream_t st);
bool policy_mlp_supported(int IN, int F1, int F2, int H);
hipError_t launch_policy_mlp(int E, int V, int IN, int F1, int F2, int H, const float* obs, const float* G, const void* W1F,
                             const void* W2f, const float* gscale, const float* b2, const float* ln2w, const float* ln2b,
                             const void* WhF, const float* hscale, const float* bh, float* heads, hipStream_t st);
hipError_t launch_policy_heads(int E, int V, int F, int H, const float* g, const float* b2, const float* lw,
                               const float* lb, const float* Wh, const float* bh, float* heads, hipStream_t st);

// The DDPG actor forward in one launch (k_sarl_actor.hip).  sarl_actor_geom(): the layout of its weight stream for a
// supported shape (items == 0 otherwise): `items` items of `rows` fragment rows of 1 KiB -- t1 pass-1 items, ng pass-2
// items, th head items; ks = fc1 k-steps of 16 the kernel is built with, mt / ht = fc2 / head output tiles of 32.
struct SarlActorGeom { int ks, mt, ht, ng, rows, t1, th, items; long long stream_bytes; };
bool sarl_actor_supported(int IN, int F1, int F2, int A);
SarlActorGeom sarl_actor_geom(int IN, int F1, int F2, int A);
hipError_t launch_sarl_actor(long long n_rows, int IN, int F1, int F2, int A, const float* x, const void* wstream,
                             const float* scales, const float* b2, const float* ln2w, const float* ln2b, const float* bmu,
                             float* logits, float* mu, hipStream_t st);
// That weight stream and its scales from the float32 weights, in two launches (k_sarl_actor_pack.hip); the workspace
// holds sarl_actor_pack_workspace() bytes (0: no such shape) and needs no initialisation.
long long sarl_actor_pack_workspace(int IN, int F1, int F2, int A);
hipError_t launch_sarl_actor_pack(int IN, int F1, int F2, int A, const float* W1, const float* b1, const float* ln1w,
                                  const float* ln1b, const float* W2, const float* Wmu, void* wstream, float* scales,
                                  void* workspace, hipStream_t st);

// k-steps of 16 that cover `width` inputs
inline int ks_of(int width) { return (width + 15) / 16; }

// Both critic kernels run a workgroup of this many wavefronts on one tile of 32 rows; each owns a quarter of every
// layer's output tiles, and the weight streams are laid out per wavefront accordingly.
constexpr int kCriticWaves = 4;

// The weight stream of k_sarl_critic: rows of 1 KiB at which its four blocks start, in stream order, and their total.
// Read by the kernel and by the launcher of its pack (a block's rows = the difference of two starts).
struct CriticLayout { long long av, fc1, fc2, fc3, rows; };
__host__ __device__ inline CriticLayout critic_layout(int KS, int KSA, int NG, int MT2, int MT3) {
    CriticLayout l;
    l.av = 0;
    l.fc1 = l.av + (long long)kCriticWaves * KSA * MT2 * 2;
    l.fc2 = l.fc1 + (long long)NG * KS * 2;
    l.fc3 = l.fc2 + (long long)kCriticWaves * (2 * NG) * MT2 * 2;
    l.rows = l.fc3 + (long long)kCriticWaves * (8 * MT2) * MT3 * 2;
    return l;
}

// The same for the three blocks of one net's stream of k_marl_critic.
struct MarlLayout { long long fc1, fc2, fc3, rows; };
__host__ __device__ inline MarlLayout marl_layout(int KS, int NG, int MT2, int MT3) {
    MarlLayout l;
    l.fc1 = 0;
    l.fc2 = l.fc1 + (long long)NG * KS * 2;
    l.fc3 = l.fc2 + (long long)kCriticWaves * (2 * NG) * MT2 * 2;
    l.rows = l.fc3 + (long long)kCriticWaves * (8 * MT2) * MT3 * 2;
    return l;
}

// The DDPG critic forward and TD target in one launch (k_sarl_critic.hip).  sarl_critic_stream_bytes(): the size of its
// weight stream for a supported shape (0 otherwise).  reward / done are read only when y is given; q and y are optional.
bool sarl_critic_supported(int IN, int F1, int F2, int F3, int A);
long long sarl_critic_stream_bytes(int IN, int F1, int F2, int F3, int A);
hipError_t launch_sarl_critic(long long n_rows, int IN, int F1, int F2, int F3, int A, const float* x, const float* a,
                              const void* wstream, const float* scales, const float* ln1w, const float* ln1b, const float* b2,
                              const float* ln2w, const float* ln2b, const float* bav, const float* b3, const float* ln3w,
                              const float* ln3b, const float* qw, const float* qb, const float* reward, const uint8_t* done,
                              float gamma, float* q, float* y, hipStream_t st);
// That weight stream and its scales from the float32 weights, in two launches (k_sarl_critic_pack.hip); the workspace
// holds sarl_critic_pack_workspace() bytes (0: no such shape) and needs no initialisation.
long long sarl_critic_pack_workspace(int IN, int F1, int F2, int F3, int A);
hipError_t launch_sarl_critic_pack(int IN, int F1, int F2, int F3, int A, const float* W1, const float* b1, const float* W2,
                                   const float* Wav, const float* W3, void* wstream, float* scales, void* workspace,
                                   hipStream_t st);

// The SAC twin global critic forward and TD target in one launch (k_marl_critic.hip): n_nets in {1, 2} plain ReLU MLPs on
// [state | action].  marl_critic_stream_bytes(): the size of ONE net's weight stream for a supported shape (0 otherwise).
// reward / done are read only when y is given, coef only with a logp pointer; q1, q2 and y are optional.
bool marl_critic_supported(int S, int A, int F1, int F2, int F3);
long long marl_critic_stream_bytes(int S, int A, int F1, int F2, int F3);
hipError_t launch_marl_critic(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticNet* nets,
                              const float* state, const float* action, const float* reward, const uint8_t* done, float gamma,
                              const float* coef, const float* logp_power, const float* logp_intent, float* q1, float* q2,
                              float* y, hipStream_t st);
// The same launch with fc1 walking the input in chunks (k_marl_critic_wide in k_marl_critic.hip), for S + A <= 512: the
// same arguments, the same weight stream (marl_layout at this shape's KS), a rule of its own that overlaps the one above.
bool marl_critic_wide_supported(int S, int A, int F1, int F2, int F3);
long long marl_critic_wide_stream_bytes(int S, int A, int F1, int F2, int F3);
hipError_t launch_marl_critic_wide(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets,
                                   const RisVecMarlCriticNet* nets, const float* state, const float* action, const float* reward,
                                   const uint8_t* done, float gamma, const float* coef, const float* logp_power,
                                   const float* logp_intent, float* q1, float* q2, float* y, hipStream_t st);
// The weight streams and scales of n_nets in {1, 2} such nets from their float32 weights, in two launches in all
// (k_marl_critic_pack.hip); the workspace holds marl_critic_pack_workspace() bytes (0: no such shape or net count) and
// needs no initialisation.  The _wide pair is the same two kernels behind marl_critic_wide_supported.
long long marl_critic_pack_workspace(int S, int A, int F1, int F2, int F3, int n_nets);
hipError_t launch_marl_critic_pack(int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticPackNet* nets,
                                   void* workspace, hipStream_t st);
long long marl_critic_wide_pack_workspace(int S, int A, int F1, int F2, int F3, int n_nets);
hipError_t launch_marl_critic_wide_pack(int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticPackNet* nets,
                                        void* workspace, hipStream_t st);

// The critic loss and its gradients in two launches (k_marl_critic_grad.hip), for the shapes of marl_critic_supported:
// the row launch walks the forward, leaves activations and deltas in the workspace and writes q1 / q2; the weight launch
// writes every gradient tensor and the loss.  marl_critic_grad_workspace(): bytes (0: no such shape, net count or n_rows).
bool marl_critic_grad_supported(int S, int A, int F1, int F2, int F3);
size_t marl_critic_grad_workspace(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets);
hipError_t launch_marl_critic_grad(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticGradNet* nets,
                                   const RisVecMarlCriticGrads* grads, const float* state, const float* action, const float* target,
                                   float* q1, float* q2, float* loss, void* workspace, hipStream_t st);

// d min(q1, q2) / d action in two launches (k_marl_critic_action_grad.hip), for the shapes of marl_critic_supported: the row
// launch walks the forward and the deltas back to the action columns of W1^T and leaves g_c and q_c in the workspace (q_c in
// q1 / q2 too where given); the select launch writes out and q_min (optional).  marl_critic_action_grad_workspace(): bytes
// (0: no such shape, net count or n_rows).
bool marl_critic_action_grad_supported(int S, int A, int F1, int F2, int F3);
size_t marl_critic_action_grad_workspace(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets);
hipError_t launch_marl_critic_action_grad(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets,
                                          const RisVecMarlCriticActionGradNet* nets, const float* state, const float* action, float scale,
                                          float* q1, float* q2, float* q_min, float* out, void* workspace, hipStream_t st);

// Every agent's local twin critics and local TD target in one launch (k_local_critics.hip): n_agents x n_nets nets of the
// shape of k_marl_critic at (S, A), nets[j n_nets + c] = agent j's net c, on agent j's columns of the batch.  Exactly one of
// action / heads is given (heads with power and A == n_agents + 2); q1, q2 and y [n_agents, n_rows] are optional.
constexpr int kLocalCriticsMaxAgents = 16;
bool local_critics_supported(int V, int S, int A, int F1, int F2, int F3);
hipError_t launch_local_critics(long long n_rows, int V, int S, int A, int F1, int F2, int F3, int n_nets,
                                const RisVecMarlCriticNet* nets, const float* obs, const float* action, const float* heads,
                                const float* power, const float* reward, const uint8_t* done, float gamma, const float* coef,
                                const float* logp_power, const float* logp_intent, float* q1, float* q2, float* y, hipStream_t st);

// target = tau online + one_minus_tau target for n_tensors <= kSoftUpdateMax tensors in one launch (k_soft_update.hip);
// the three arrays are host arrays, copied into the kernel's argument block.
constexpr int kSoftUpdateMax = 32;
hipError_t launch_soft_update(int n_tensors, const float* const* online, float* const* target, const int64_t* numel,
                              float tau, float one_minus_tau, hipStream_t st);

// clip_grad_norm_ + Adam + the target blend of n_groups networks over n_tensors tensors in two launches, one without
// RISVEC_ADAM_CLIP (k_adam.hip).  All pointers are device memory; a workgroup owns kAdamChunk elements of one tensor.
constexpr int kAdamChunk = RISVEC_ADAM_CHUNK;
struct AdamLaunch {
    const RisVecAdamTensor* tensors;
    const RisVecAdamGroup* groups;
    const int32_t* block_tensor;
    double* partials;
    float* norms;
    double bc1;
    float omb1, b2, omb2, bc2_sqrt, eps, tau, omt;
    int n_tensors, n_groups, n_blocks;
    uint32_t flags;
};
hipError_t launch_adam_step(const AdamLaunch& a, hipStream_t st);

int episode_partial_rows(int E);
hipError_t launch_episode_clear(int E, int V, double* acc, hipStream_t st);
hipError_t launch_episode_accumulate(int E, int V, const float* metrics, const float* reward, const float* power_w,
                                     float user_clip, double* acc, hipStream_t st);
hipError_t launch_episode_summary(int E, int V, int n_steps, const double* acc, const float* metrics, double* per_env,
                                  double* partial, double* summary, hipStream_t st);

// bytes per env row of state.theta_idx: the candidate index of every theta element, padded to a multiple of 32
// (four 8-element tiles: the pair sweep reads and writes the indices of four tiles per request)
__host__ __device__ inline int theta_idx_stride(int n_ris) { return (n_ris + 31) / 32 * 32; }
hipError_t launch_theta_from_index(const RisVecState& s, hipStream_t st);

// risvec_last_kernel(): the launchers of the step path and the BCD sweep name the kernel they dispatched (per thread)
void note_kernel(const char* fmt, ...);
// risvec_last_theta_by_index(): note_kernel() clears it, the step launcher sets it after naming its kernel
void note_theta_by_index(bool by_index);
// risvec_last_h_r_rebuilt(): likewise
void note_h_r_rebuilt(bool rebuilt);
// risvec_last_h_r_heads(): likewise
void note_h_r_heads(bool heads);
// state.steer_ang -> heads [E,V,M/16] c128 by steer_head(), M % 16 == 0 (k_step_gen.hip)
hipError_t launch_steer_heads(const RisVecState& s, double* heads, hipStream_t st);
// state.steer_ang / state.z_r -> out [E,V,M] c64 by steer_chunk(), M % 16 == 0 (k_step_gen.hip)
hipError_t launch_h_r_from_steer(const RisVecState& s, float* out, hipStream_t st);

// risvec_force_forms(): the test / A/B override of the dispatch rules.  Read by the step selector (plan_step) and
// launch_colsum only.
const RisVecForce& forced_forms();
// `rule` unless the override field forces the form on or off
inline bool forced_or(int32_t field, bool rule) { return field == RISVEC_BY_RULE ? rule : field == RISVEC_FORCE_ON; }

// Launch `kernel(args)` with lds_bytes of dynamic LDS; beyond 64 KiB the kernel's limit is raised first.
template <typename Args>
hipError_t launch_dynamic_lds(void (*kernel)(Args), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args& args) {
    if (lds_bytes > 64 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds_bytes);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args);
    return hipGetLastError();
}

// The <MT2, MT3> = <fc2 / 128, fc3 / 128> instantiation of a critic kernel, fc2 in {128, 256, 512}, fc3 in {128, 256}:
// f(std::integral_constant<int, MT2>, std::integral_constant<int, MT3>) launches it.
template <typename F>
hipError_t dispatch_mt2_mt3(int F2, int F3, F&& f) {
    auto f3 = [&](auto mt2) {
        return F3 == 256 ? f(mt2, std::integral_constant<int, 2>{}) : f(mt2, std::integral_constant<int, 1>{});
    };
    switch (F2) {
        case 128: return f3(std::integral_constant<int, 1>{});
        case 256: return f3(std::integral_constant<int, 2>{});
        case 512: return f3(std::integral_constant<int, 4>{});
    }
    return hipErrorInvalidValue;
}

inline Dims dims_of(const RisVecState& s) {
    return Dims{s.n_envs, s.n_veh, s.n_ris, s.control_bit, (long long)s.env_offset};
}

}  // namespace risvec
