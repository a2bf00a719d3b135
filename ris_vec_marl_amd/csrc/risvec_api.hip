// C ABI of librisvec.so (declared in include/risvec.h): argument validation, error
// strings, and dispatch to the kernel launchers.  Nothing here computes on the CPU:
// every entry point either launches HIP kernels or fails with an error code.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "risvec_launch.hpp"
#include "risvec_sarl.hpp"
#include "risvec_step.hpp"

namespace {

thread_local char g_err[512] = "";
thread_local char g_kernel[160] = "";
thread_local int g_theta_by_index = 0;
thread_local int g_h_r_rebuilt = 0;
thread_local int g_h_r_heads = 0;
RisVecForce g_force{};                  // risvec_force_forms(): all RISVEC_BY_RULE

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// `pre`: what stands in front of a field's name, "" or an Indexed("nets", c).s
#define REQ_PTR_IN(pre, ptr, name)                                                           \
    do {                                                                                     \
        if ((ptr) == nullptr) return fail(RISVEC_ERR_ARG, "%s: %s%s is NULL", fn, pre, name); \
        if (!aligned16(ptr)) return fail(RISVEC_ERR_ARG, "%s: %s%s is not 16-byte aligned", fn, pre, name); \
    } while (0)
#define REQ_PTR(ptr, name) REQ_PTR_IN("", ptr, name)
// float data that is read float by float wherever it does not start on 16 bytes: float alignment is all it needs
#define OPT_F32_IN(pre, ptr, name)                                                           \
    do {                                                                                     \
        if (reinterpret_cast<uintptr_t>(ptr) & 3u)                                           \
            return fail(RISVEC_ERR_ARG, "%s: %s%s is not 4-byte aligned", fn, pre, name);    \
    } while (0)
#define REQ_F32_IN(pre, ptr, name)                                                           \
    do {                                                                                     \
        if ((ptr) == nullptr) return fail(RISVEC_ERR_ARG, "%s: %s%s is NULL", fn, pre, name); \
        OPT_F32_IN(pre, ptr, name);                                                          \
    } while (0)
#define OPT_PTR(ptr, name)                                                                   \
    do {                                                                                     \
        if ((ptr) != nullptr && !aligned16(ptr))                                             \
            return fail(RISVEC_ERR_ARG, "%s: %s is not 16-byte aligned", fn, name);          \
    } while (0)

// "nets[3]." and its like
struct Indexed {
    char s[32];
    Indexed(const char* array, int i) { snprintf(s, sizeof(s), "%s[%d].", array, i); }
};

// n_envs and n_veh, as a state carries them or as an entry point without a state takes them
int check_envs_veh(const char* fn, int32_t n_envs, int32_t n_veh) {
    if (n_envs < 1) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d must be >= 1", fn, n_envs);
    if (n_veh < 1 || n_veh > RISVEC_MAX_VEH)
        return fail(RISVEC_ERR_SHAPE, "%s: n_veh=%d outside [1,%d]", fn, n_veh, RISVEC_MAX_VEH);
    return RISVEC_OK;
}

// A weight stream of another shape than the call's.  `have` is printed as its type has it: int64_t where the argument is
// one, size_t in the pack entry points.
template <typename T>
int check_wstream_bytes(const char* fn, const char* pre, T have, long long want) {
    if (have == (T)want) return RISVEC_OK;
    if (std::is_signed<T>::value)
        return fail(RISVEC_ERR_ARG, "%s: %swstream_bytes=%lld, this shape's weight stream has %lld", fn, pre, (long long)have, want);
    return fail(RISVEC_ERR_ARG, "%s: %swstream_bytes=%zu, this shape's weight stream has %lld", fn, pre, (size_t)have, want);
}

// The workspace of a pack entry point: `need` bytes for this `what` ("shape" or "call"), as `ws_fn` states them
int check_workspace_bytes(const char* fn, size_t have, size_t need, const char* what, const char* ws_fn) {
    if (have < need)
        return fail(RISVEC_ERR_ARG, "%s: workspace_bytes=%zu, this %s needs %zu (%s)", fn, have, what, need, ws_fn);
    return RISVEC_OK;
}

// The net table of risvec_marl_critic (count = n_nets) and risvec_local_critics (count = n_agents * n_nets)
int check_critic_nets(const char* fn, const RisVecMarlCriticNet* nets, int count, long long need_bytes) {
    for (int c = 0; c < count; ++c) {
        const RisVecMarlCriticNet& n = nets[c];
        const Indexed pre("nets", c);
        if (int rc = check_wstream_bytes(fn, pre.s, n.wstream_bytes, need_bytes)) return rc;
        REQ_PTR_IN(pre.s, n.wstream, "wstream"); REQ_PTR_IN(pre.s, n.scales, "scales"); REQ_PTR_IN(pre.s, n.b1, "b1");
        REQ_PTR_IN(pre.s, n.b2, "b2"); REQ_PTR_IN(pre.s, n.b3, "b3"); REQ_PTR_IN(pre.s, n.qw, "qw");
        if (!n.qb) return fail(RISVEC_ERR_ARG, "%s: %sqb is NULL", fn, pre.s);
    }
    return RISVEC_OK;
}

// The outputs and the TD epilogue of the same two: at least one output, and every input that an output asks for
int check_critic_outputs(const char* fn, int n_nets, const float* reward, const uint8_t* done, float gamma, const float* coef,
                         const float* logp_power, const float* logp_intent, const float* q1, const float* q2, const float* y) {
    if (!q1 && !q2 && !y) return fail(RISVEC_ERR_ARG, "%s: q1, q2 and y are all NULL", fn);
    if (q2 && n_nets != 2) return fail(RISVEC_ERR_ARG, "%s: q2 needs n_nets == 2", fn);
    if (y && (!reward || !done)) return fail(RISVEC_ERR_ARG, "%s: y needs reward and done", fn);
    if ((logp_power || logp_intent) && !coef) return fail(RISVEC_ERR_ARG, "%s: logp_power / logp_intent need coef", fn);
    if ((logp_power || logp_intent) && !y) return fail(RISVEC_ERR_ARG, "%s: logp_power / logp_intent need y", fn);
    if (!std::isfinite(gamma)) return fail(RISVEC_ERR_ARG, "%s: gamma=%g must be finite", fn, (double)gamma);
    return RISVEC_OK;
}

// every entry point opens with this; `params` = false for the ones that take no RisVecParams (p is NULL there)
int check_common(const char* fn, const RisVecState* s, const RisVecParams* p, bool params = true) {
    if (params && !p) return fail(RISVEC_ERR_ARG, "%s: params is NULL", fn);
    if (!s) return fail(RISVEC_ERR_ARG, "%s: state is NULL", fn);
    if (s->abi_version != RISVEC_ABI_VERSION || s->struct_bytes != sizeof(RisVecState))
        return fail(RISVEC_ERR_ARG, "%s: RisVecState ABI mismatch (version %u/%u, bytes %u/%zu)", fn,
                    s->abi_version, (unsigned)RISVEC_ABI_VERSION, s->struct_bytes, sizeof(RisVecState));
    if (p && (p->abi_version != RISVEC_ABI_VERSION || p->struct_bytes != sizeof(RisVecParams)))
        return fail(RISVEC_ERR_ARG, "%s: RisVecParams ABI mismatch (version %u/%u, bytes %u/%zu)", fn,
                    p->abi_version, (unsigned)RISVEC_ABI_VERSION, p->struct_bytes, sizeof(RisVecParams));
    if (int rc = check_envs_veh(fn, s->n_envs, s->n_veh)) return rc;
    if (s->n_ris < 1 || s->n_ris > 2048)
        return fail(RISVEC_ERR_SHAPE, "%s: n_ris=%d outside [1,2048]", fn, s->n_ris);
    if (s->control_bit < 0 || s->control_bit > 6)
        return fail(RISVEC_ERR_SHAPE, "%s: control_bit=%d outside [0,6]", fn, s->control_bit);
    if ((long long)s->n_envs * s->n_veh * s->n_ris > (1LL << 40))
        return fail(RISVEC_ERR_SHAPE, "%s: E*V*M too large", fn);
    if (s->env_offset < 0 || s->env_offset + s->n_envs > 0xFFFFFFFFLL)
        return fail(RISVEC_ERR_SHAPE, "%s: env_offset+n_envs must fit 32 bits", fn);
    if (p && (p->n_lanes < 1 || p->n_lanes > RISVEC_MAX_LANES))
        return fail(RISVEC_ERR_SHAPE, "%s: n_lanes=%d outside [1,%d]", fn, p->n_lanes, RISVEC_MAX_LANES);
    return RISVEC_OK;
}

int finish(const char* fn, hipError_t err) {
    if (err != hipSuccess) return fail(RISVEC_ERR_LAUNCH, "%s: %s", fn, hipGetErrorString(err));
    return RISVEC_OK;
}

// The arguments every step entry point shares.  A T-step entry point passes `tj` as well: n_steps and the records are
// checked, and *tj becomes the records its kernels write (an obs record needs RISVEC_STEP_OBS).
int check_step(const char* fn, const RisVecState* s, const float* action, const int32_t* partner,
               const int32_t* n_groups, const int32_t* arrivals, uint32_t flags, bool fused, int32_t n_steps = 1,
               const RisVecTraj* traj = nullptr, RisVecTraj* tj = nullptr) {
    if (tj) {
        if (n_steps < 1 || n_steps > (1 << 20)) return fail(RISVEC_ERR_ARG, "%s: n_steps=%d outside [1, 2^20]", fn, n_steps);
        if (flags & (RISVEC_STEP_REUSE_COLSUM | RISVEC_STEP_REUSE_SSUM | RISVEC_STEP_REUSE_IDX | RISVEC_STEP_STEER | RISVEC_STEP_THETA_BY_INDEX))
            return fail(RISVEC_ERR_ARG, "%s: the BCD / steering flags (0x%x) are not accepted by the multi-step launch", fn, flags);
        *tj = RisVecTraj{nullptr, nullptr, nullptr};
        if (traj) {
            OPT_PTR(traj->reward, "traj.reward"); OPT_PTR(traj->obs, "traj.obs"); OPT_PTR(traj->metrics, "traj.metrics");
            *tj = *traj;
            if (!(flags & RISVEC_STEP_OBS)) tj->obs = nullptr;
        }
    }
    REQ_PTR(action, "action"); REQ_PTR(partner, "partner"); REQ_PTR(n_groups, "n_groups");
    OPT_PTR(arrivals, "arrivals");
    REQ_PTR(s->gain, "state.gain"); REQ_PTR(s->data_buf, "state.data_buf"); REQ_PTR(s->mec_q, "state.mec_q");
    REQ_PTR(s->rate, "state.rate"); REQ_PTR(s->data_t, "state.data_t"); REQ_PTR(s->data_p, "state.data_p");
    REQ_PTR(s->reward, "state.reward"); REQ_PTR(s->over_power, "state.over_power");
    REQ_PTR(s->metrics, "state.metrics");
    if (flags & RISVEC_STEP_OBS) REQ_PTR(s->obs, "state.obs");
    if (flags & RISVEC_STEP_POWER_W) REQ_PTR(s->power_w, "state.power_w");
    if (flags & ~(uint32_t)(RISVEC_STEP_METRICS | RISVEC_STEP_POWER_W | RISVEC_STEP_POLICY_ACTION | RISVEC_STEP_OBS |
                            RISVEC_STEP_REUSE_COLSUM | RISVEC_STEP_REUSE_SSUM | RISVEC_STEP_REUSE_IDX | RISVEC_STEP_STEER |
                            RISVEC_STEP_THETA_BY_INDEX))
        return fail(RISVEC_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags);
    if (flags & RISVEC_STEP_STEER) {
        if (!fused) return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_STEER needs the fused entry points", fn);
        REQ_PTR(s->z_r, "state.z_r");
    }
    if (fused) {
        REQ_PTR(s->h_r, "state.h_r"); REQ_PTR(s->theta, "state.theta"); REQ_PTR(s->b, "state.b");
        REQ_PTR(s->pl, "state.pl"); OPT_PTR(s->h_d, "state.h_d");
    }
    return RISVEC_OK;
}

// RISVEC_STEP_THETA_IDX_CURRENT, RISVEC_STEP_H_R_STEER_CURRENT and RISVEC_STEP_STEER_HEADS_CURRENT, accepted by
// risvec_step_fused and the fused form of risvec_step_ring only (check_step refuses them as unknown bits everywhere else):
// checks what they need and returns the flags check_step sees
int check_idx_current(const char* fn, const RisVecState* s, bool fused, uint32_t* flags) {
    if (*flags & RISVEC_STEP_STEER_HEADS_CURRENT) {
        if (!fused) return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_STEER_HEADS_CURRENT is a hint to the fused forms (this one rebuilds no h_r)", fn);
        if (!(*flags & RISVEC_STEP_H_R_STEER_CURRENT))
            return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_STEER_HEADS_CURRENT needs RISVEC_STEP_H_R_STEER_CURRENT (the heads serve the "
                        "rebuilt rows only)", fn);
        *flags &= ~(uint32_t)RISVEC_STEP_STEER_HEADS_CURRENT;
    }
    if (*flags & RISVEC_STEP_H_R_STEER_CURRENT) {
        if (!fused) return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_H_R_STEER_CURRENT is a hint to the fused forms (this one reads no h_r)", fn);
        if (*flags & RISVEC_STEP_STEER)
            return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_H_R_STEER_CURRENT and RISVEC_STEP_STEER exclude each other", fn);
        OPT_PTR(s->steer_ang, "state.steer_ang"); OPT_PTR(s->z_r, "state.z_r");
        *flags &= ~(uint32_t)RISVEC_STEP_H_R_STEER_CURRENT;
    }
    if (!(*flags & RISVEC_STEP_THETA_IDX_CURRENT)) return RISVEC_OK;
    if (!fused) return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_THETA_IDX_CURRENT is a hint to the fused forms (this one reads no theta)", fn);
    REQ_PTR(s->theta_idx, "state.theta_idx");
    if (s->control_bit != 3)
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_THETA_IDX_CURRENT needs control_bit = 3 (candidate indices exist for 2^b = 8 "
                    "only), got %d", fn, s->control_bit);
    *flags &= ~(uint32_t)RISVEC_STEP_THETA_IDX_CURRENT;
    return RISVEC_OK;
}

// the transition-store arguments of risvec_step_ring / risvec_step_fused_3gpp, checked and translated
int check_ring(const char* fn, const RisVecState* s, const RisVecStepRing* ring, uint32_t flags, risvec::StepRing* out) {
    const uint32_t need = RISVEC_STEP_POLICY_ACTION | RISVEC_STEP_OBS;
    if ((flags & need) != need)
        return fail(RISVEC_ERR_ARG, "%s: flags must hold RISVEC_STEP_POLICY_ACTION | RISVEC_STEP_OBS (the ring stores the raw policy "
                    "output and both observations)", fn);
    if (flags & (RISVEC_STEP_STEER | RISVEC_STEP_THETA_BY_INDEX | RISVEC_STEP_REUSE_COLSUM | RISVEC_STEP_REUSE_SSUM | RISVEC_STEP_REUSE_IDX))
        return fail(RISVEC_ERR_ARG, "%s: steering / theta-by-index / BCD flags (0x%x) are not accepted here", fn, flags);
    const RisVecReplay& rb = ring->rb;
    const int V = s->n_veh;
    if (V != 4 && V != 8 && V != 16)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: n_veh=%d (the fused transition store exists for 4, 8 and 16 vehicles)", fn, V);
    if (rb.n_agents != V || rb.input_shape != 5 || rb.n_actions != V + 2)
        return fail(RISVEC_ERR_SHAPE, "%s: the ring must have n_agents = n_veh = %d, input_shape = 5, n_actions = %d (got %d, %d, %d)",
                    fn, V, V + 2, rb.n_agents, rb.input_shape, rb.n_actions);
    if (rb.mem_size < s->n_envs) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d transitions do not fit mem_size=%lld", fn, s->n_envs,
                                             (long long)rb.mem_size);
    if (ring->mem_cntr < 0) return fail(RISVEC_ERR_ARG, "%s: mem_cntr < 0", fn);
    REQ_PTR(rb.state_memory, "ring.state_memory"); REQ_PTR(rb.action_memory, "ring.action_memory");
    REQ_PTR(rb.reward_global_memory, "ring.reward_global_memory"); REQ_PTR(rb.reward_local_memory, "ring.reward_local_memory");
    REQ_PTR(rb.new_state_memory, "ring.new_state_memory"); REQ_PTR(rb.terminal_memory, "ring.terminal_memory");
    REQ_PTR(rb.mask_memory, "ring.mask_memory"); REQ_PTR(ring->probs, "ring.probs"); OPT_PTR(ring->mask, "ring.mask");
    REQ_PTR(s->obs, "state.obs");
    *out = risvec::StepRing{rb.state_memory, rb.action_memory, rb.reward_global_memory, rb.reward_local_memory, rb.new_state_memory,
                       rb.terminal_memory, rb.mask_memory, ring->probs, ring->mask, (long long)(ring->mem_cntr % rb.mem_size),
                       (long long)rb.mem_size, ring->done ? 1 : 0};
    return RISVEC_OK;
}

// the model and the injected fading draws of a 3GPP gain; `pre` + name is what the caller calls a draw, `free_fn` serves 'free'
int check_3gpp(const char* fn, int32_t model, const float* u_los, const float* z_shadow, const float* small, const char* pre,
               const char* free_fn) {
    if (model != RISVEC_CH_3GPP_UMI && model != RISVEC_CH_3GPP_UMA && model != RISVEC_CH_OTHER)
        return fail(RISVEC_ERR_ARG, "%s: model=%d is not a 3GPP/other model (%s 'free')", fn, model, free_fn);
    const struct { const float* ptr; const char* name; } draws[3] = {{u_los, "u_los"}, {z_shadow, "z_shadow"}, {small, "small"}};
    int n_inj = 0;
    for (const auto& d : draws) {
        if (!aligned16(d.ptr)) return fail(RISVEC_ERR_ARG, "%s: %s%s is not 16-byte aligned", fn, pre, d.name);
        n_inj += d.ptr != nullptr;
    }
    if (n_inj != 0 && n_inj != 3)
        return fail(RISVEC_ERR_ARG, "%s: %su_los, z_shadow, small must all be given or all be NULL", fn, pre);
    return RISVEC_OK;
}

// the arguments of the fused 3GPP entry points besides the ring (`tj`: as for check_step)
int check_step_3gpp(const char* fn, const RisVecState* s, const RisVecParams* p, int32_t model, const float* action,
                    const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals, const RisVecFading* fading,
                    uint32_t flags, int32_t n_steps = 1, const RisVecTraj* traj = nullptr, RisVecTraj* tj = nullptr) {
    if (int rc = check_common(fn, s, p)) return rc;
    const RisVecFading fd = fading ? *fading : RisVecFading{nullptr, nullptr, nullptr};
    if (int rc = check_3gpp(fn, model, fd.u_los, fd.z_shadow, fd.small, "fading.", "the RIS step entry points serve")) return rc;
    if (flags & ~(uint32_t)(RISVEC_STEP_METRICS | RISVEC_STEP_POWER_W | RISVEC_STEP_OBS | RISVEC_STEP_POLICY_ACTION))
        return fail(RISVEC_ERR_ARG, "%s: flags 0x%x: only METRICS / POWER_W / OBS / POLICY_ACTION are accepted (steering, "
                    "theta-by-index and BCD are forms of the RIS step)", fn, flags);
    if (int rc = check_step(fn, s, action, partner, n_groups, arrivals, flags, false, n_steps, traj, tj)) return rc;
    REQ_PTR(s->pos, "state.pos");
    return RISVEC_OK;
}

risvec::Chan3gpp chan_3gpp(const RisVecState* s, int32_t model, const RisVecFading* fading, uint32_t chan_counter) {
    risvec::Chan3gpp c{s->pos, nullptr, nullptr, nullptr, chan_counter, model};
    if (fading && fading->u_los) { c.u_los = fading->u_los; c.z_shadow = fading->z_shadow; c.small = fading->small; }
    return c;
}

}  // namespace

namespace risvec {
void note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
    g_theta_by_index = 0;
    g_h_r_rebuilt = 0;
    g_h_r_heads = 0;
}

void note_theta_by_index(bool by_index) { g_theta_by_index = by_index ? 1 : 0; }

void note_h_r_rebuilt(bool rebuilt) { g_h_r_rebuilt = rebuilt ? 1 : 0; }

void note_h_r_heads(bool heads) { g_h_r_heads = heads ? 1 : 0; }

const RisVecForce& forced_forms() { return g_force; }
}  // namespace risvec

extern "C" {

uint32_t risvec_abi_version(void) { return RISVEC_ABI_VERSION; }

const char* risvec_last_kernel(void) { return g_kernel; }

int risvec_last_theta_by_index(void) { return g_theta_by_index; }

int risvec_last_pipe_walk(void) { return risvec::last_pipe_walk(); }

int risvec_last_h_r_rebuilt(void) { return g_h_r_rebuilt; }

int risvec_last_h_r_heads(void) { return g_h_r_heads; }

int risvec_last_gen_groups_per_wave(void) { return g_h_r_rebuilt ? risvec::last_gen_launch_groups_per_wave() : 0; }

const char* risvec_last_error(void) { return g_err; }

const char* risvec_step_kernel(const RisVecState* s, uint32_t flags, int32_t form) {
    const char* fn = "risvec_step_kernel";
    thread_local char name[sizeof(risvec::StepPlan::name)];
    if (check_common(fn, s, nullptr, false)) return nullptr;
    if (form < RISVEC_FORM_CACHED || form > RISVEC_FORM_FUSED_MULTI) {
        fail(RISVEC_ERR_ARG, "%s: form=%d is not a RISVEC_FORM_*", fn, form);
        return nullptr;
    }
    const risvec::StepPlan pl = risvec::plan_step(*s, flags, form);
    if (pl.family == risvec::StepPlan::NONE) {
        fail(RISVEC_ERR_UNSUPPORTED, "%s: form %d has no kernel at n_veh=%d, n_ris=%d (flags 0x%x)", fn, form, s->n_veh, s->n_ris,
             flags);
        return nullptr;
    }
    std::memcpy(name, pl.name, sizeof(name));
    return name;
}

int risvec_force_forms(const RisVecForce* f) {
    const char* fn = "risvec_force_forms";
    if (!f) {
        g_force = RisVecForce{};
        return RISVEC_OK;
    }
    if (f->abi_version != RISVEC_ABI_VERSION || f->struct_bytes != sizeof(RisVecForce))
        return fail(RISVEC_ERR_ARG, "%s: RisVecForce ABI mismatch (version %u/%u, bytes %u/%zu)", fn, f->abi_version,
                    (unsigned)RISVEC_ABI_VERSION, f->struct_bytes, sizeof(RisVecForce));
    for (int32_t v : {f->lat, f->lat_nt, f->lat_alt, f->pipe_nt, f->colsum_nt, f->pipe_rev})
        if (v != RISVEC_BY_RULE && v != RISVEC_FORCE_OFF && v != RISVEC_FORCE_ON)
            return fail(RISVEC_ERR_ARG, "%s: %d is not RISVEC_BY_RULE / RISVEC_FORCE_OFF / RISVEC_FORCE_ON", fn, v);
    if (f->lat_epw != 0 && f->lat_epw != 1 && f->lat_epw != 2 && f->lat_epw != 4)
        return fail(RISVEC_ERR_ARG, "%s: lat_epw=%d is not 0 (by rule), 1, 2 or 4", fn, f->lat_epw);
    if (f->pipe_waves < 0) return fail(RISVEC_ERR_ARG, "%s: pipe_waves=%d is not 0 (by rule) or a wavefront count", fn, f->pipe_waves);
    g_force = *f;
    return RISVEC_OK;
}

void risvec_default_params(RisVecParams* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->abi_version = RISVEC_ABI_VERSION;
    p->struct_bytes = sizeof(RisVecParams);
    p->bandwidth_mhz = 1.0f;                                           // ENV:72
    p->noise_power = (float)(std::pow(10.0, (-174.0 - 30.0) / 10.0) * 1.0e6);   // ENV:74-76
    p->p_max = 1.0f;                                                   // ENV:125
    p->power_scale = 0.7f;                                             // ENV:555
    p->qos_enable = 1; p->r_min_bpshz = 0.20f; p->d_max_s = 0.10f; p->qos_penalty = 5.0f;   // ENV:79-82
    p->time_fast = 1e-3f;                                              // ENV:102
    p->k_cpu = 1e-28f;                                                 // ENV:104
    p->f_local_max = 1.0e9f; p->f_edge_max = 2.0e9f;                   // ENV:108-109
    p->cycles_per_bit = 500.0f; p->cpu_share_floor = 0.10f;            // ENV:111-113
    p->w_d = 0.5f; p->w_e = 3.0f; p->reward_clip = 50.0f;              // ENV:138-143
    p->arrival_rate = 3.0f;                                            // ENV:156
    {   // Poisson(3) CDF, float64 -> float32
        double pk = std::exp(-3.0), cdf = 0.0;
        for (int k = 0; k < RISVEC_POISSON_TABLE; ++k) {
            cdf += pk;
            p->poisson_cdf[k] = (float)(cdf < 1.0 ? cdf : 1.0);
            pk *= 3.0 / (double)(k + 1);
        }
    }
    p->fc_ghz = 3.5f; p->shadow_std_los = 4.0f; p->shadow_std_nlos = 7.0f;   // ENV:186-188
    p->rician_k_db = 0.0f; p->veh_ant_gain = 3.0f;                     // ENV:189, 96
    p->n_lanes = 4;
    p->time_slow = 0.1; p->width = 400.0; p->height = 400.0;           // ENV:101
    const double up[4] = {(400 + 3.5 / 2) / 2.0, (400 + 3.5 + 3.5 / 2) / 2.0, (800 + 3.5 / 2) / 2.0,
                          (800 + 3.5 + 3.5 / 2) / 2.0};                // marl_train_bcd.py:446
    const double dn[4] = {(400 - 3.5 - 3.5 / 2) / 2.0, (400 - 3.5 / 2) / 2.0, (800 - 3.5 - 3.5 / 2) / 2.0,
                          (800 - 3.5 / 2) / 2.0};                      // marl_train_bcd.py:447
    for (int i = 0; i < 4; ++i) {
        p->lanes_up[i] = up[i]; p->lanes_left[i] = up[i];
        p->lanes_down[i] = dn[i]; p->lanes_right[i] = dn[i];
    }
}

int risvec_reset(const RisVecState* s, const RisVecParams* p, const int32_t* spawn_ints,
                 const int32_t* buf0, uint64_t seed, uint32_t counter, risvec_stream_t stream) {
    const char* fn = "risvec_reset";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(s->pos, "state.pos"); REQ_PTR(s->dir, "state.dir"); REQ_PTR(s->vel, "state.vel");
    REQ_PTR(s->data_buf, "state.data_buf");
    OPT_PTR(spawn_ints, "spawn_ints"); OPT_PTR(buf0, "buf0");
    if ((spawn_ints == nullptr) != (buf0 == nullptr))
        return fail(RISVEC_ERR_ARG, "%s: spawn_ints and buf0 must both be given or both be NULL", fn);
    if (p->n_lanes != 4)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: the reference spawn rule is defined for 4 lanes per direction", fn);
    return finish(fn, risvec::launch_reset(*s, *p, spawn_ints, buf0, seed, counter, (hipStream_t)stream));
}

int risvec_mobility(const RisVecState* s, const RisVecParams* p, const float* u_turn, int32_t* n_used,
                    uint64_t seed, uint32_t counter, risvec_stream_t stream) {
    const char* fn = "risvec_mobility";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(s->pos, "state.pos"); REQ_PTR(s->dir, "state.dir"); REQ_PTR(s->vel, "state.vel");
    OPT_PTR(u_turn, "u_turn"); OPT_PTR(n_used, "n_used");
    if (p->n_lanes > 4)     // a move may draw 2 * n_lanes numbers; a u_turn row and the two Philox sites hold 8
        return fail(RISVEC_ERR_UNSUPPORTED,
                    "%s: n_lanes=%d: a move may need 2*n_lanes turn draws and u_turn rows hold 8 (at most 4 lanes per direction)",
                    fn, p->n_lanes);
    return finish(fn, risvec::launch_mobility(*s, *p, u_turn, n_used, seed, counter, (hipStream_t)stream));
}

int risvec_geometry(const RisVecState* s, const RisVecParams* p, risvec_stream_t stream) {
    const char* fn = "risvec_geometry";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(s->pos, "state.pos"); REQ_PTR(s->dist_r, "state.dist_r"); REQ_PTR(s->ang_r, "state.ang_r");
    OPT_PTR(s->z_r, "state.z_r"); OPT_PTR(s->steer_ang, "state.steer_ang");
    REQ_PTR(s->pl, "state.pl"); REQ_PTR(s->h_r, "state.h_r");
    OPT_PTR(s->c_col, "state.c_col");
    if (int rc = finish(fn, risvec::launch_geometry(*s, *p, (hipStream_t)stream))) return rc;
    if (s->c_col) {                      // keep the BCD column-sum cache in step with h_r
        REQ_PTR(s->b, "state.b");
        return finish(fn, risvec::launch_colsum(*s, (hipStream_t)stream));
    }
    return RISVEC_OK;
}

int risvec_h_r_from_steer(const RisVecState* s, float* out, risvec_stream_t stream) {
    const char* fn = "risvec_h_r_from_steer";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(s->steer_ang, "state.steer_ang"); REQ_PTR(s->z_r, "state.z_r"); REQ_PTR(out, "out");
    if (s->n_ris % 16 != 0)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: n_ris=%d is not a multiple of 16 (rows are rebuilt in 16-element chunks)", fn, s->n_ris);
    return finish(fn, risvec::launch_h_r_from_steer(*s, out, (hipStream_t)stream));
}

int risvec_steer_heads(const RisVecState* s, double* heads, risvec_stream_t stream) {
    const char* fn = "risvec_steer_heads";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(s->steer_ang, "state.steer_ang"); REQ_PTR(heads, "heads");
    if (s->n_ris % 16 != 0)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: n_ris=%d is not a multiple of 16 (a head stands in front of a 16-element chunk)", fn,
                    s->n_ris);
    return finish(fn, risvec::launch_steer_heads(*s, heads, (hipStream_t)stream));
}

int risvec_gain(const RisVecState* s, const RisVecParams* p, risvec_stream_t stream) {
    const char* fn = "risvec_gain";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(s->h_r, "state.h_r"); REQ_PTR(s->theta, "state.theta"); REQ_PTR(s->b, "state.b");
    REQ_PTR(s->pl, "state.pl"); REQ_PTR(s->gain, "state.gain"); OPT_PTR(s->h_d, "state.h_d");
    return finish(fn, risvec::launch_gain(*s, *p, (hipStream_t)stream));
}

int risvec_gain_3gpp(const RisVecState* s, const RisVecParams* p, int32_t model, const float* u_los,
                     const float* z_shadow, const float* small, uint64_t seed, uint32_t counter,
                     risvec_stream_t stream) {
    const char* fn = "risvec_gain_3gpp";
    if (int rc = check_common(fn, s, p)) return rc;
    if (int rc = check_3gpp(fn, model, u_los, z_shadow, small, "", "use risvec_gain for")) return rc;
    REQ_PTR(s->pos, "state.pos"); REQ_PTR(s->gain, "state.gain");
    return finish(fn, risvec::launch_gain_3gpp(*s, *p, model, u_los, z_shadow, small, seed, counter,
                                               (hipStream_t)stream));
}

int risvec_colsum(const RisVecState* s, risvec_stream_t stream) {
    const char* fn = "risvec_colsum";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(s->h_r, "state.h_r"); REQ_PTR(s->b, "state.b"); REQ_PTR(s->c_col, "state.c_col");
    return finish(fn, risvec::launch_colsum(*s, (hipStream_t)stream));
}

int risvec_bcd(const RisVecState* s, const RisVecParams* p, int32_t* idx_out, uint32_t flags,
               risvec_stream_t stream) {
    const char* fn = "risvec_bcd";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(s->h_r, "state.h_r"); REQ_PTR(s->theta, "state.theta"); REQ_PTR(s->b, "state.b");
    REQ_PTR(s->c_col, "state.c_col");
    OPT_PTR(idx_out, "idx_out");
    OPT_PTR(s->s_sum, "state.s_sum");
    OPT_PTR(s->theta_idx, "state.theta_idx");
    if (flags & ~(uint32_t)(RISVEC_BCD_REUSE_COLSUM | RISVEC_BCD_REUSE_SSUM | RISVEC_BCD_REUSE_IDX | RISVEC_BCD_NO_THETA))
        return fail(RISVEC_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags);
    if ((flags & RISVEC_BCD_NO_THETA) && (!(flags & RISVEC_BCD_REUSE_IDX) || s->control_bit != 3))
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_BCD_NO_THETA needs RISVEC_BCD_REUSE_IDX and control_bit = 3", fn);
    if ((flags & RISVEC_BCD_REUSE_SSUM) && !s->s_sum)
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_BCD_REUSE_SSUM needs state.s_sum", fn);
    if ((flags & RISVEC_BCD_REUSE_IDX) && !s->theta_idx)
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_BCD_REUSE_IDX needs state.theta_idx", fn);
    return finish(fn, risvec::launch_bcd(*s, *p, idx_out, (flags & RISVEC_BCD_REUSE_COLSUM) != 0,
                                         (flags & RISVEC_BCD_REUSE_SSUM) != 0, (flags & RISVEC_BCD_REUSE_IDX) != 0,
                                         (flags & RISVEC_BCD_NO_THETA) == 0, (hipStream_t)stream));
}

int risvec_theta_from_index(const RisVecState* s, risvec_stream_t stream) {
    const char* fn = "risvec_theta_from_index";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(s->theta, "state.theta"); REQ_PTR(s->theta_idx, "state.theta_idx");
    if (s->control_bit != 3) return fail(RISVEC_ERR_UNSUPPORTED, "%s: candidate indices exist for control_bit = 3 only", fn);
    return finish(fn, risvec::launch_theta_from_index(*s, (hipStream_t)stream));
}

int risvec_theta_by_index_supported(int32_t n_veh, int32_t n_ris) {
    return risvec::theta_by_index_supported(n_veh, n_ris) ? 1 : 0;
}

int risvec_set_phase(const RisVecState* s, const float* angle, risvec_stream_t stream) {
    const char* fn = "risvec_set_phase";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(angle, "angle"); REQ_PTR(s->theta, "state.theta");
    return finish(fn, risvec::launch_set_phase(*s, angle, (hipStream_t)stream));
}

int risvec_random_phase(const RisVecState* s, const int32_t* idx, uint64_t seed, uint32_t counter,
                        risvec_stream_t stream) {
    const char* fn = "risvec_random_phase";
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    OPT_PTR(idx, "idx"); REQ_PTR(s->theta, "state.theta"); OPT_PTR(s->theta_idx, "state.theta_idx");
    return finish(fn, risvec::launch_random_phase(*s, idx, seed, counter, (hipStream_t)stream));
}

int risvec_step(const RisVecState* s, const RisVecParams* p, const float* action, const int32_t* partner,
                const int32_t* n_groups, const int32_t* arrivals, uint64_t seed, uint32_t counter,
                uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_step";
    if (int rc = check_common(fn, s, p)) return rc;
    if (int rc = check_step(fn, s, action, partner, n_groups, arrivals, flags, false)) return rc;
    if (flags & RISVEC_STEP_THETA_BY_INDEX)
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_THETA_BY_INDEX is a form of the fused entry points (this one reads no theta)", fn);
    return finish(fn, risvec::launch_step(*s, *p, action, partner, n_groups, arrivals, seed, counter, flags,
                                          false, (hipStream_t)stream));
}

int risvec_data_rate(const RisVecState* s, const RisVecParams* p, const float* p_off, const int32_t* partner,
                     const int32_t* n_groups, float* rate_out, risvec_stream_t stream) {
    const char* fn = "risvec_data_rate";
    if (int rc = check_common(fn, s, p)) return rc;
    REQ_PTR(p_off, "p_off"); REQ_PTR(partner, "partner"); REQ_PTR(n_groups, "n_groups");
    REQ_PTR(rate_out, "rate_out"); REQ_PTR(s->gain, "state.gain");
    return finish(fn, risvec::launch_data_rate(*s, *p, p_off, partner, n_groups, rate_out, (hipStream_t)stream));
}

int risvec_step_fused(const RisVecState* s, const RisVecParams* p, const float* action,
                      const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals,
                      uint64_t seed, uint32_t counter, uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_step_fused";
    if (int rc = check_common(fn, s, p)) return rc;
    uint32_t known = flags;
    if (int rc = check_idx_current(fn, s, true, &known)) return rc;
    if (int rc = check_step(fn, s, action, partner, n_groups, arrivals, known, true)) return rc;
    if (flags & RISVEC_STEP_THETA_BY_INDEX) {                  // theta as the last sweep's candidate indices (no sweep here)
        REQ_PTR(s->theta_idx, "state.theta_idx");
        if (s->control_bit != 3 || !risvec::theta_by_index_supported(s->n_veh, s->n_ris) || (flags & RISVEC_STEP_STEER))
            return fail(RISVEC_ERR_UNSUPPORTED, "%s: no theta-by-index form of the fused step for control_bit=%d, n_veh=%d, "
                        "n_ris=%d%s", fn, s->control_bit, s->n_veh, s->n_ris, (flags & RISVEC_STEP_STEER) ? " with RISVEC_STEP_STEER" : "");
    }
    return finish(fn, risvec::launch_step(*s, *p, action, partner, n_groups, arrivals, seed, counter, flags,
                                          true, (hipStream_t)stream));
}

int risvec_step_fused_multi(const RisVecState* s, const RisVecParams* p, int32_t n_steps, const float* actions,
                            const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals, uint64_t seed,
                            uint32_t counter, uint32_t flags, const RisVecTraj* traj, risvec_stream_t stream) {
    const char* fn = "risvec_step_fused_multi";
    if (int rc = check_common(fn, s, p)) return rc;
    RisVecTraj tj;
    if (int rc = check_step(fn, s, actions, partner, n_groups, arrivals, flags, true, n_steps, traj, &tj)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const risvec::StepArgs a = risvec::make_step_args(*s, actions, partner, n_groups, arrivals, seed, counter, flags);
    // `traj`, not `tj`: this kernel writes an obs record even without RISVEC_STEP_OBS (the other T-step paths drop it); kept as is
    const hipError_t err = risvec::launch_step_fused_multi(*s, *p, a, n_steps, traj, st);
    if (err != hipErrorNotSupported) return finish(fn, err);
    // Shapes without a compile-time fused kernel: step 0 through the single fused launch (gains computed and stored, its
    // records copied out), steps 1 .. T-1 in ONE launch on those stored gains (h_r / theta cannot change inside the call,
    // so they are the gains T fused launches would recompute): bit-identical to T risvec_step_fused calls.
    const long long ev = (long long)s->n_envs * s->n_veh;
    const hipError_t e1 = risvec::launch_step(*s, *p, actions, partner, n_groups, arrivals, seed, counter, flags, true, st);
    if (e1 != hipSuccess) return finish(fn, e1);
    hipError_t e2 = hipSuccess;
    if (tj.reward) e2 = hipMemcpyAsync(tj.reward, s->reward, ev * 4, hipMemcpyDeviceToDevice, st);
    if (e2 == hipSuccess && tj.obs) e2 = hipMemcpyAsync(tj.obs, s->obs, ev * 20, hipMemcpyDeviceToDevice, st);
    if (e2 == hipSuccess && tj.metrics)
        e2 = hipMemcpyAsync(tj.metrics, s->metrics, (size_t)s->n_envs * RISVEC_METRICS * 4, hipMemcpyDeviceToDevice, st);
    if (e2 != hipSuccess) return finish(fn, e2);
    if (n_steps == 1) return RISVEC_OK;
    const risvec::StepArgs rest = risvec::make_step_args(*s, actions + 2 * ev, partner, n_groups,
                                                         arrivals ? arrivals + ev : nullptr, seed, counter + 1u, flags);
    if (tj.reward) tj.reward += ev;
    if (tj.obs) tj.obs += ev * 5;
    if (tj.metrics) tj.metrics += (long long)s->n_envs * RISVEC_METRICS;
    return finish(fn, risvec::launch_step_multi(*s, *p, rest, n_steps - 1, &tj, st));
}

int risvec_step_multi(const RisVecState* s, const RisVecParams* p, int32_t n_steps, const float* actions,
                      const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals, uint64_t seed,
                      uint32_t counter, uint32_t flags, const RisVecTraj* traj, risvec_stream_t stream) {
    const char* fn = "risvec_step_multi";
    if (int rc = check_common(fn, s, p)) return rc;
    RisVecTraj tj;
    if (int rc = check_step(fn, s, actions, partner, n_groups, arrivals, flags, false, n_steps, traj, &tj)) return rc;
    const risvec::StepArgs a = risvec::make_step_args(*s, actions, partner, n_groups, arrivals, seed, counter, flags);
    return finish(fn, risvec::launch_step_multi(*s, *p, a, n_steps, &tj, (hipStream_t)stream));
}

// the SARL parameter block of risvec_sarl_step / risvec_sarl_rollout
static int check_sarl_params(const char* fn, const RisVecSarlParams* p) {
    if (!p) return fail(RISVEC_ERR_ARG, "%s: params is NULL", fn);
    if (p->abi_version != RISVEC_ABI_VERSION || p->struct_bytes != sizeof(RisVecSarlParams))
        return fail(RISVEC_ERR_ARG, "%s: RisVecSarlParams ABI mismatch (version %u/%u, bytes %u/%zu)", fn,
                    p->abi_version, (unsigned)RISVEC_ABI_VERSION, p->struct_bytes, sizeof(RisVecSarlParams));
    return RISVEC_OK;
}

// the five arrays of a SARL ring (buffer.py:7-11), all required
static int check_sarl_ring(const char* fn, const RisVecSarlRollout* r) {
    REQ_PTR(r->state_memory, "ring.state_memory"); REQ_PTR(r->action_memory, "ring.action_memory");
    REQ_PTR(r->reward_memory, "ring.reward_memory"); REQ_PTR(r->new_state_memory, "ring.new_state_memory");
    REQ_PTR(r->terminal_memory, "ring.terminal_memory");
    if (r->mem_size < 1) return fail(RISVEC_ERR_SHAPE, "%s: mem_size=%lld must be >= 1", fn, (long long)r->mem_size);
    return RISVEC_OK;
}

// the state arrays a SARL step reads or writes; `obs`: state.obs as well
static int check_sarl_state(const char* fn, const RisVecState* s, bool obs) {
    REQ_PTR(s->h_r, "state.h_r"); REQ_PTR(s->theta, "state.theta"); REQ_PTR(s->b, "state.b"); REQ_PTR(s->pl, "state.pl");
    REQ_PTR(s->gain, "state.gain"); REQ_PTR(s->data_buf, "state.data_buf"); REQ_PTR(s->rate, "state.rate");
    REQ_PTR(s->data_t, "state.data_t"); REQ_PTR(s->data_p, "state.data_p"); REQ_PTR(s->reward, "state.reward");
    REQ_PTR(s->over_power, "state.over_power"); REQ_PTR(s->over_data, "state.over_data");
    REQ_PTR(s->metrics, "state.metrics");
    if (obs) REQ_PTR(s->obs, "state.obs");
    return RISVEC_OK;
}

// RISVEC_STEP_OBS is the one flag of the SARL entry points
static int check_sarl_flags(const char* fn, uint32_t flags) {
    if (flags & ~(uint32_t)RISVEC_STEP_OBS) return fail(RISVEC_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags);
    return RISVEC_OK;
}

int risvec_sarl_step(const RisVecState* s, const RisVecSarlParams* p, const float* action_power,
                     const float* action_phase, const int32_t* arrivals, uint64_t seed, uint32_t counter,
                     uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_sarl_step";
    if (int rc = check_sarl_params(fn, p)) return rc;
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    REQ_PTR(action_power, "action_power"); OPT_PTR(action_phase, "action_phase"); OPT_PTR(arrivals, "arrivals");
    if (int rc = check_sarl_state(fn, s, (flags & RISVEC_STEP_OBS) != 0)) return rc;
    if (int rc = check_sarl_flags(fn, flags)) return rc;
    return finish(fn, risvec::launch_sarl_step(*s, *p, action_power, action_phase, arrivals, seed, counter, flags,
                                               (hipStream_t)stream));
}

int risvec_sarl_rollout_supported(int32_t n_veh, int32_t n_ris) { return risvec::sarl_rollout_covers(n_veh, n_ris) ? 1 : 0; }

int risvec_sarl_rollout(const RisVecState* s, const RisVecSarlParams* p, const RisVecSarlRollout* r, const int32_t* arrivals,
                        uint64_t seed, uint32_t counter, uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_sarl_rollout";
    if (int rc = check_sarl_params(fn, p)) return rc;
    if (!r) return fail(RISVEC_ERR_ARG, "%s: rollout is NULL", fn);
    if (r->struct_bytes != sizeof(RisVecSarlRollout))
        return fail(RISVEC_ERR_ARG, "%s: RisVecSarlRollout ABI mismatch (bytes %u/%zu)", fn, r->struct_bytes, sizeof(RisVecSarlRollout));
    if (int rc = check_common(fn, s, nullptr, false)) return rc;
    if (int rc = check_sarl_flags(fn, flags)) return rc;
    if (!risvec::sarl_rollout_covers(s->n_veh, s->n_ris))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: no one-launch rollout kernel at n_veh=%d, n_ris=%d (n_veh in {4, 8, 16}, even "
                    "n_ris with n_veh <= n_ris <= 256); use the staged path: map the action on the host side, then "
                    "risvec_sarl_step", fn, s->n_veh, s->n_ris);
    REQ_PTR(r->mu, "rollout.mu"); OPT_PTR(r->ou_x, "rollout.ou_x"); OPT_PTR(r->z, "rollout.z");
    REQ_PTR(r->action, "rollout.action"); REQ_PTR(r->phase, "rollout.phase"); REQ_PTR(r->obs_full, "rollout.obs_full");
    OPT_PTR(arrivals, "arrivals");
    if (r->z && !r->ou_x) return fail(RISVEC_ERR_ARG, "%s: rollout.z (injected draws) needs rollout.ou_x", fn);
    if (r->ou_x) {
        if (!(r->ou_dt >= 0.0f) || !std::isfinite(r->ou_dt))
            return fail(RISVEC_ERR_ARG, "%s: ou_dt=%g must be finite and >= 0", fn, (double)r->ou_dt);
        if (r->ou_env_offset < 0 || r->ou_env_offset + s->n_envs > 0xFFFFFFFFLL)
            return fail(RISVEC_ERR_SHAPE, "%s: ou_env_offset+n_envs must fit 32 bits", fn);
    }
    if (int rc = check_sarl_state(fn, s, true)) return rc;
    if (r->state_memory || r->action_memory || r->reward_memory || r->new_state_memory || r->terminal_memory) {
        if (int rc = check_sarl_ring(fn, r)) return rc;
        if (r->mem_size < s->n_envs)
            return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d transitions do not fit mem_size=%lld", fn, s->n_envs, (long long)r->mem_size);
        if (r->mem_cntr < 0) return fail(RISVEC_ERR_ARG, "%s: mem_cntr < 0", fn);
    }
    const hipError_t err = risvec::launch_sarl_rollout(*s, *p, *r, arrivals, seed, counter, (hipStream_t)stream);
    if (err == hipErrorNotSupported)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: no one-launch rollout kernel at n_veh=%d, n_ris=%d; use the staged path "
                    "(risvec_sarl_step)", fn, s->n_veh, s->n_ris);
    return finish(fn, err);
}

int risvec_sarl_replay_sample(const RisVecSarlRollout* ring, int32_t state_dims, int32_t n_actions, int64_t max_mem,
                              int32_t batch, const int64_t* idx, uint64_t seed, uint32_t counter, float* states,
                              float* actions, float* rewards, float* states_, uint8_t* dones, int64_t* idx_out,
                              risvec_stream_t stream) {
    const char* fn = "risvec_sarl_replay_sample";
    if (!ring) return fail(RISVEC_ERR_ARG, "%s: ring is NULL", fn);
    if (ring->struct_bytes != sizeof(RisVecSarlRollout))
        return fail(RISVEC_ERR_ARG, "%s: RisVecSarlRollout ABI mismatch (bytes %u/%zu)", fn, ring->struct_bytes, sizeof(RisVecSarlRollout));
    if (int rc = check_sarl_ring(fn, ring)) return rc;
    if (state_dims < 1 || n_actions < 1)
        return fail(RISVEC_ERR_SHAPE, "%s: state_dims=%d and n_actions=%d must be >= 1", fn, state_dims, n_actions);
    if (batch < 1) return fail(RISVEC_ERR_SHAPE, "%s: batch=%d must be >= 1", fn, batch);
    if (max_mem < 1 || max_mem > ring->mem_size)
        return fail(RISVEC_ERR_ARG, "%s: max_mem=%lld outside [1, mem_size=%lld] (sampling an empty buffer?)", fn,
                    (long long)max_mem, (long long)ring->mem_size);
    OPT_PTR(idx, "idx"); OPT_PTR(idx_out, "idx_out");
    REQ_PTR(states, "states"); REQ_PTR(actions, "actions"); REQ_PTR(rewards, "rewards"); REQ_PTR(states_, "states_");
    REQ_PTR(dones, "dones");
    return finish(fn, risvec::launch_sarl_replay_sample(*ring, state_dims, n_actions, max_mem, batch, idx, seed, counter, states,
                                                        actions, rewards, states_, dones, idx_out, (hipStream_t)stream));
}

int risvec_step_fused_bcd(const RisVecState* s, const RisVecParams* p, const float* action,
                          const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals,
                          uint64_t seed, uint32_t counter, uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_step_fused_bcd";
    if (int rc = check_common(fn, s, p)) return rc;
    if (int rc = check_step(fn, s, action, partner, n_groups, arrivals, flags, true)) return rc;
    REQ_PTR(s->c_col, "state.c_col");
    OPT_PTR(s->theta_idx, "state.theta_idx");
    if ((flags & RISVEC_STEP_REUSE_IDX) && !s->theta_idx)
        return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_REUSE_IDX needs state.theta_idx", fn);
    if (flags & RISVEC_STEP_THETA_BY_INDEX) {
        if (!(flags & RISVEC_STEP_REUSE_IDX) || s->control_bit != 3)
            return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_THETA_BY_INDEX needs RISVEC_STEP_REUSE_IDX and control_bit = 3", fn);
        if (!risvec::theta_by_index_supported(s->n_veh, s->n_ris))
            return fail(RISVEC_ERR_UNSUPPORTED, "%s: no theta-by-index form of the fused step at n_veh=%d, n_ris=%d", fn,
                        s->n_veh, s->n_ris);
        if (flags & RISVEC_STEP_STEER)
            return fail(RISVEC_ERR_ARG, "%s: RISVEC_STEP_THETA_BY_INDEX and RISVEC_STEP_STEER exclude each other", fn);
    }
    return finish(fn, risvec::launch_step_fused_bcd(*s, *p, action, partner, n_groups, arrivals, seed,
                                                    counter, flags, (hipStream_t)stream));
}

int risvec_step_ring(const RisVecState* s, const RisVecParams* p, const RisVecStepRing* ring, const float* action,
                     const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals, uint64_t seed,
                     uint32_t counter, uint32_t flags, int32_t fused, risvec_stream_t stream) {
    const char* fn = "risvec_step_ring";
    if (int rc = check_common(fn, s, p)) return rc;
    if (!ring) return fail(RISVEC_ERR_ARG, "%s: ring is NULL", fn);
    uint32_t known = flags;
    if (int rc = check_idx_current(fn, s, fused != 0, &known)) return rc;
    if (int rc = check_step(fn, s, action, partner, n_groups, arrivals, known, fused != 0)) return rc;
    risvec::StepRing r;
    if (int rc = check_ring(fn, s, ring, known, &r)) return rc;
    const int V = s->n_veh;
    const hipError_t err = risvec::launch_step(*s, *p, action, partner, n_groups, arrivals, seed, counter, flags, fused != 0,
                                               (hipStream_t)stream, &r);
    if (err == hipErrorNotSupported)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: no fused-gains kernel with the transition store at n_veh=%d, n_ris=%d (use "
                    "risvec_step_fused + risvec_replay_store_policy)", fn, V, s->n_ris);
    return finish(fn, err);
}

int risvec_step_fused_3gpp(const RisVecState* s, const RisVecParams* p, int32_t model, const float* action,
                           const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals,
                           const RisVecFading* fading, uint64_t seed, uint32_t counter, uint32_t chan_counter,
                           uint32_t flags, const RisVecStepRing* ring, risvec_stream_t stream) {
    const char* fn = "risvec_step_fused_3gpp";
    if (int rc = check_step_3gpp(fn, s, p, model, action, partner, n_groups, arrivals, fading, flags)) return rc;
    risvec::StepArgs a = risvec::make_step_args(*s, action, partner, n_groups, arrivals, seed, counter, flags);
    if (ring)
        if (int rc = check_ring(fn, s, ring, flags, &a.ring)) return rc;
    const hipError_t err = risvec::launch_step_3gpp(*s, *p, a, chan_3gpp(s, model, fading, chan_counter),
                                                    ring ? RISVEC_FORM_FUSED_RING : RISVEC_FORM_FUSED, 1, RisVecTraj{},
                                                    (hipStream_t)stream);
    if (err == hipErrorNotSupported)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: no 3GPP step kernel at n_veh=%d%s", fn, s->n_veh, ring ? " with the ring" : "");
    return finish(fn, err);
}

int risvec_step_fused_3gpp_multi(const RisVecState* s, const RisVecParams* p, int32_t model, int32_t n_steps,
                                 const float* actions, const int32_t* partner, const int32_t* n_groups,
                                 const int32_t* arrivals, const RisVecFading* fading, uint64_t seed, uint32_t counter,
                                 uint32_t chan_counter, const RisVecTraj* traj, uint32_t flags, risvec_stream_t stream) {
    const char* fn = "risvec_step_fused_3gpp_multi";
    RisVecTraj tj;
    if (int rc = check_step_3gpp(fn, s, p, model, actions, partner, n_groups, arrivals, fading, flags, n_steps, traj, &tj)) return rc;
    const risvec::StepArgs a = risvec::make_step_args(*s, actions, partner, n_groups, arrivals, seed, counter, flags);
    const hipError_t err = risvec::launch_step_3gpp(*s, *p, a, chan_3gpp(s, model, fading, chan_counter),
                                                    RISVEC_FORM_FUSED_MULTI, n_steps, tj, (hipStream_t)stream);
    if (err == hipErrorNotSupported)
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: no 3GPP T-step kernel at n_veh=%d", fn, s->n_veh);
    return finish(fn, err);
}

// ---------------------------------------------------------------------------------------------
// NOMA grouping stage (f2)
// ---------------------------------------------------------------------------------------------
void risvec_noma_default_params(RisVecNomaParams* p, int32_t n_veh) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->min_pair_target = n_veh / 4 > 1 ? n_veh / 4 : 1;               // TRAIN:489
    p->mwm_backoff_rounds = 5; p->mwm_allow_singles = 1;               // TRAIN:440, 436
    p->qos_enable = 0; p->relax_topk_step = 1;                         // TRAIN:750 (Config default), 728
    p->freeze_group_in_episode = 1; p->freeze_recalc_every = 0;        // TRAIN:738-739
    p->mask_enable = 1;                                                // TRAIN:498
    p->mwm_accept_quantile = 0.10; p->mwm_accept_q_step = 0.05;        // TRAIN:439, 441
    p->completion_min_quantile = 0.30;                                 // TRAIN:282
    p->score_w_delta_db = 1.0; p->score_w_history = 0.3f;              // TRAIN:716-717
    p->abs_gain_min_db = -HUGE_VAL;                                    // TRAIN:723
    p->qos_soft_penalty = 6.0; p->qos_R_min = 0.0;                     // TRAIN:172, 751
    p->noise_power = std::pow(10.0, -174.0 / 10.0) / 1000.0 * 1.0e6;   // ENV:72-76
    p->P_max = 1.0;                                                    // ENV:125
    p->relax_tau_factor = 0.95; p->tau_back_floor_db = 3.0;            // TRAIN:729, 1499
    p->freeze_reward_drop_ratio = 0.05; p->freeze_unstick_prob = 0.0;  // TRAIN:741, 740
    p->pair_hist_decay = 0.97f;                                        // TRAIN:719
}

int64_t risvec_noma_scratch_bytes(int32_t n_envs, int32_t n_veh) {
    if (n_envs < 1 || n_veh < 1 || n_veh > RISVEC_NOMA_MAX_VEH) return 0;
    return risvec::noma_scratch_bytes(n_envs, n_veh);
}

static int check_noma(const char* fn, const RisVecNomaState* ns) {
    if (!ns) return fail(RISVEC_ERR_ARG, "%s: noma state is NULL", fn);
    if (ns->n_envs < 1) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d must be >= 1", fn, ns->n_envs);
    if (ns->n_veh < 1 || ns->n_veh > RISVEC_NOMA_MAX_VEH)
        return fail(RISVEC_ERR_SHAPE, "%s: n_veh=%d outside [1,%d]", fn, ns->n_veh, RISVEC_NOMA_MAX_VEH);
    if (ns->env_offset < 0 || ns->env_offset + ns->n_envs > 0xFFFFFFFFLL)
        return fail(RISVEC_ERR_SHAPE, "%s: env_offset+n_envs must fit 32 bits", fn);
    return RISVEC_OK;
}

int risvec_noma_begin_episode(const RisVecNomaState* ns, risvec_stream_t stream) {
    const char* fn = "risvec_noma_begin_episode";
    if (int rc = check_noma(fn, ns)) return rc;
    REQ_PTR(ns->hist, "noma.hist"); REQ_PTR(ns->streak, "noma.streak"); REQ_PTR(ns->flags, "noma.flags");
    REQ_PTR(ns->pending, "noma.pending");
    return finish(fn, risvec::launch_noma_begin_episode(*ns, (hipStream_t)stream));
}

int risvec_noma_mask(const RisVecNomaState* ns, const float* gain, const double* gdb15, double q_now, int32_t K_now,
                     risvec_stream_t stream) {
    const char* fn = "risvec_noma_mask";
    if (int rc = check_noma(fn, ns)) return rc;
    OPT_PTR(gdb15, "gdb15");
    if (!gdb15) REQ_PTR(gain, "gain");
    REQ_PTR(ns->tau, "noma.tau");
    if (K_now >= 1) REQ_PTR(ns->mask, "noma.mask");
    if (!(q_now >= 0.0 && q_now <= 1.0)) return fail(RISVEC_ERR_ARG, "%s: q_now=%g outside [0,1]", fn, q_now);
    return finish(fn, risvec::launch_noma_mask(*ns, gain, gdb15, q_now, K_now, (hipStream_t)stream));
}

static int check_noma_state(const char* fn, const RisVecNomaState* ns) {
    REQ_PTR(ns->hist, "noma.hist"); REQ_PTR(ns->streak, "noma.streak"); REQ_PTR(ns->partner, "noma.partner");
    REQ_PTR(ns->n_groups, "noma.n_groups"); REQ_PTR(ns->last_global, "noma.last_global");
    REQ_PTR(ns->best_global, "noma.best_global"); REQ_PTR(ns->flags, "noma.flags");
    REQ_PTR(ns->pending, "noma.pending");
    return RISVEC_OK;
}

static int noma_group_impl(const char* fn, const RisVecNomaState* ns, const RisVecNomaParams* np, const float* gain,
                           const double* gdb12, const float* p_off01, int p01_raw, int32_t use_mask, int32_t K_back,
                           const double* tau_back, const float* prev_global, int32_t prev_global_stride, int32_t i_step,
                           const float* u_unstick, uint64_t seed, uint32_t counter, int32_t* info_out,
                           risvec_stream_t stream) {
    if (int rc = check_noma(fn, ns)) return rc;
    if (!np) return fail(RISVEC_ERR_ARG, "%s: params is NULL", fn);
    REQ_PTR(gain, "gain"); OPT_PTR(gdb12, "gdb12"); OPT_PTR(p_off01, "p_off01"); REQ_PTR(tau_back, "tau_back");
    OPT_PTR(u_unstick, "u_unstick"); OPT_PTR(info_out, "info_out");
    if (int rc = check_noma_state(fn, ns)) return rc;
    if (np->qos_enable && !p_off01) return fail(RISVEC_ERR_ARG, "%s: qos_enable needs p_off01", fn);
    if (np->mask_enable && use_mask) REQ_PTR(ns->mask, "noma.mask");
    if (prev_global && prev_global_stride < 1)
        return fail(RISVEC_ERR_ARG, "%s: prev_global_stride=%d must be >= 1", fn, prev_global_stride);
    if (prev_global && (reinterpret_cast<uintptr_t>(prev_global) & 3u))
        return fail(RISVEC_ERR_ARG, "%s: prev_global is not 4-byte aligned", fn);
    if (K_back < 0) return fail(RISVEC_ERR_ARG, "%s: K_back=%d must be >= 0", fn, K_back);
    const long long need = risvec::noma_scratch_bytes(ns->n_envs, ns->n_veh);
    if (need > 0 && (!ns->scratch || ns->scratch_bytes < need))
        return fail(RISVEC_ERR_ARG, "%s: noma.scratch holds %lld bytes, risvec_noma_scratch_bytes(%d, %d) = %lld", fn,
                    ns->scratch ? (long long)ns->scratch_bytes : 0LL, ns->n_envs, ns->n_veh, need);
    if (need > 0) REQ_PTR(ns->scratch, "noma.scratch");
    if (np->mwm_backoff_rounds < 0 || np->mwm_backoff_rounds > 64)
        return fail(RISVEC_ERR_ARG, "%s: mwm_backoff_rounds=%d outside [0,64]", fn, np->mwm_backoff_rounds);
    return finish(fn, risvec::launch_noma_group(*ns, *np, gain, gdb12, p_off01, p01_raw, use_mask, K_back, tau_back,
                                                prev_global, prev_global_stride, i_step, u_unstick, seed, counter,
                                                info_out, (hipStream_t)stream));
}

int risvec_noma_group(const RisVecNomaState* ns, const RisVecNomaParams* np, const float* gain, const double* gdb12,
                      const float* p_off01, int32_t use_mask, int32_t K_back, const double* tau_back,
                      const float* prev_global, int32_t prev_global_stride, int32_t i_step, const float* u_unstick,
                      uint64_t seed, uint32_t counter, int32_t* info_out, risvec_stream_t stream) {
    return noma_group_impl("risvec_noma_group", ns, np, gain, gdb12, p_off01, 0, use_mask, K_back, tau_back, prev_global,
                           prev_global_stride, i_step, u_unstick, seed, counter, info_out, stream);
}

int risvec_noma_group_raw(const RisVecNomaState* ns, const RisVecNomaParams* np, const float* gain, const double* gdb12,
                          const float* power_raw, int32_t use_mask, int32_t K_back, const double* tau_back,
                          const float* prev_global, int32_t prev_global_stride, int32_t i_step, const float* u_unstick,
                          uint64_t seed, uint32_t counter, int32_t* info_out, risvec_stream_t stream) {
    return noma_group_impl("risvec_noma_group_raw", ns, np, gain, gdb12, power_raw, 1, use_mask, K_back, tau_back,
                           prev_global, prev_global_stride, i_step, u_unstick, seed, counter, info_out, stream);
}

int risvec_noma_flush(const RisVecNomaState* ns, const RisVecNomaParams* np, risvec_stream_t stream) {
    const char* fn = "risvec_noma_flush";
    if (int rc = check_noma(fn, ns)) return rc;
    if (!np) return fail(RISVEC_ERR_ARG, "%s: params is NULL", fn);
    if (int rc = check_noma_state(fn, ns)) return rc;
    return finish(fn, risvec::launch_noma_flush(*ns, np->pair_hist_decay, (hipStream_t)stream));
}

// ---------------------------------------------------------------------------------------------
// replay ring buffer + marshalling (f3)
// ---------------------------------------------------------------------------------------------
static int check_replay(const char* fn, const RisVecReplay* rb) {
    if (!rb) return fail(RISVEC_ERR_ARG, "%s: replay is NULL", fn);
    if (rb->n_agents < 1 || rb->n_agents > RISVEC_MAX_VEH || rb->input_shape < 1 || rb->n_actions < 1)
        return fail(RISVEC_ERR_SHAPE, "%s: n_agents=%d input_shape=%d n_actions=%d", fn, rb->n_agents, rb->input_shape,
                    rb->n_actions);
    if (rb->mem_size < 1) return fail(RISVEC_ERR_SHAPE, "%s: mem_size=%lld must be >= 1", fn, (long long)rb->mem_size);
    REQ_PTR(rb->state_memory, "replay.state_memory"); REQ_PTR(rb->action_memory, "replay.action_memory");
    REQ_PTR(rb->reward_global_memory, "replay.reward_global_memory");
    REQ_PTR(rb->reward_local_memory, "replay.reward_local_memory");
    REQ_PTR(rb->new_state_memory, "replay.new_state_memory"); REQ_PTR(rb->terminal_memory, "replay.terminal_memory");
    REQ_PTR(rb->mask_memory, "replay.mask_memory");
    return RISVEC_OK;
}

static int replay_store_impl(const char* fn, const RisVecReplay* rb, int64_t mem_cntr, int32_t n, const float* state,
                             const float* action, const float* power_raw, const float* probs, const float* reward_g,
                             int32_t reward_g_stride, const float* reward_l, const float* state_, const uint8_t* done,
                             int32_t done_all, const uint8_t* mask, float* state_carry, risvec_stream_t stream) {
    if (int rc = check_replay(fn, rb)) return rc;
    if (n < 1 || n > rb->mem_size)
        return fail(RISVEC_ERR_SHAPE, "%s: n=%d outside [1, mem_size=%lld] (a batch may not overwrite itself)", fn, n,
                    (long long)rb->mem_size);
    if (mem_cntr < 0) return fail(RISVEC_ERR_ARG, "%s: mem_cntr=%lld must be >= 0", fn, (long long)mem_cntr);
    if (reward_g_stride < 1) return fail(RISVEC_ERR_ARG, "%s: reward_g_stride=%d must be >= 1", fn, reward_g_stride);
    REQ_PTR(state, "state"); REQ_PTR(reward_l, "reward_l"); REQ_PTR(state_, "state_");
    if (action) {
        REQ_PTR(action, "action");
    } else {
        REQ_PTR(power_raw, "power_raw"); REQ_PTR(probs, "probs");
        if (rb->n_actions != rb->n_agents + 2)
            return fail(RISVEC_ERR_SHAPE, "%s: the policy-output form needs n_actions = n_agents + 2 (got %d, %d)", fn,
                        rb->n_actions, rb->n_agents);
    }
    OPT_PTR(state_carry, "state_carry"); OPT_PTR(mask, "mask");
    if (state_carry == state || state_carry == state_)
        return fail(RISVEC_ERR_ARG, "%s: state_carry must not alias state / state_ (other lanes are reading them)", fn);
    if (!reward_g || (reinterpret_cast<uintptr_t>(reward_g) & 3u))
        return fail(RISVEC_ERR_ARG, "%s: reward_g is NULL or not 4-byte aligned", fn);
    return finish(fn, risvec::launch_replay_store(*rb, mem_cntr, n, state, action, power_raw, probs, reward_g, reward_g_stride, reward_l,
                                                  state_, done, done_all, mask, state_carry, (hipStream_t)stream));
}

int risvec_replay_store(const RisVecReplay* rb, int64_t mem_cntr, int32_t n, const float* state, const float* action,
                        const float* reward_g, int32_t reward_g_stride, const float* reward_l, const float* state_,
                        const uint8_t* done, int32_t done_all, const uint8_t* mask, float* state_carry,
                        risvec_stream_t stream) {
    if (!action && rb && rb->mem_size >= 1 && rb->n_agents >= 1 && rb->state_memory)   // (a malformed rb is reported first)
        return fail(RISVEC_ERR_ARG, "risvec_replay_store: action is NULL");
    return replay_store_impl("risvec_replay_store", rb, mem_cntr, n, state, action, nullptr, nullptr, reward_g, reward_g_stride,
                             reward_l, state_, done, done_all, mask, state_carry, stream);
}

int risvec_replay_store_policy(const RisVecReplay* rb, int64_t mem_cntr, int32_t n, const float* state,
                               const float* power_raw, const float* probs, const float* reward_g, int32_t reward_g_stride,
                               const float* reward_l, const float* state_, const uint8_t* done, int32_t done_all,
                               const uint8_t* mask, float* state_carry, risvec_stream_t stream) {
    return replay_store_impl("risvec_replay_store_policy", rb, mem_cntr, n, state, nullptr, power_raw, probs, reward_g,
                             reward_g_stride, reward_l, state_, done, done_all, mask, state_carry, stream);
}

int risvec_replay_sample(const RisVecReplay* rb, int64_t max_mem, int32_t batch, const int64_t* idx, uint64_t seed,
                         uint32_t counter, float* states, float* actions, float* rewards_g, float* rewards_l,
                         float* states_, uint8_t* dones, float* masks, int64_t* idx_out, risvec_stream_t stream) {
    const char* fn = "risvec_replay_sample";
    if (int rc = check_replay(fn, rb)) return rc;
    if (batch < 1) return fail(RISVEC_ERR_SHAPE, "%s: batch=%d must be >= 1", fn, batch);
    if (max_mem < 1 || max_mem > rb->mem_size)
        return fail(RISVEC_ERR_ARG, "%s: max_mem=%lld outside [1, mem_size=%lld] (sampling an empty buffer?)", fn,
                    (long long)max_mem, (long long)rb->mem_size);
    OPT_PTR(idx, "idx"); OPT_PTR(idx_out, "idx_out");
    REQ_PTR(states, "states"); REQ_PTR(actions, "actions"); REQ_PTR(rewards_g, "rewards_g");
    REQ_PTR(rewards_l, "rewards_l"); REQ_PTR(states_, "states_"); REQ_PTR(dones, "dones"); REQ_PTR(masks, "masks");
    return finish(fn, risvec::launch_replay_sample(*rb, max_mem, batch, idx, seed, counter, states, actions, rewards_g,
                                                   rewards_l, states_, dones, masks, idx_out, (hipStream_t)stream));
}

// cpu_share_floor as the marshalling kernels take it: within [0, 0.95]
static float clamp_share_floor(float f) { return f < 0.0f ? 0.0f : (f > 0.95f ? 0.95f : f); }

int risvec_marshal_actions(int32_t n_envs, int32_t n_veh, const float* power_raw, const float* probs,
                           float cpu_share_floor, float* action_env, float* p_off01, float* action_store,
                           risvec_stream_t stream) {
    const char* fn = "risvec_marshal_actions";
    if (int rc = check_envs_veh(fn, n_envs, n_veh)) return rc;
    REQ_PTR(power_raw, "power_raw"); OPT_PTR(probs, "probs"); OPT_PTR(action_env, "action_env");
    OPT_PTR(p_off01, "p_off01"); OPT_PTR(action_store, "action_store");
    if (action_store && !probs) return fail(RISVEC_ERR_ARG, "%s: action_store needs probs", fn);
    if ((long long)n_envs * n_veh * (n_veh + 2) >= (1LL << 31))
        return fail(RISVEC_ERR_SHAPE, "%s: n_envs*n_veh*(n_veh+2) must stay below 2^31", fn);
    const float fl = clamp_share_floor(cpu_share_floor);
    return finish(fn, risvec::launch_marshal_actions(n_envs, n_veh, power_raw, probs, fl, action_env, p_off01,
                                                     action_store, (hipStream_t)stream));
}

int risvec_policy_sample(int32_t n_envs, int32_t n_veh, int64_t env_offset, const float* heads, const uint8_t* mask,
                         const float* tau, const uint8_t* hard, const float* eps, const float* expo, uint64_t seed,
                         uint32_t counter, float cpu_share_floor, float* power_raw, float* probs, float* onehot,
                         float* action_env, float* p_off01, float* action_store, risvec_stream_t stream) {
    const char* fn = "risvec_policy_sample";
    if (int rc = check_envs_veh(fn, n_envs, n_veh)) return rc;
    if (env_offset < 0 || env_offset + n_envs > 0xFFFFFFFFLL)
        return fail(RISVEC_ERR_SHAPE, "%s: env_offset+n_envs must fit 32 bits", fn);
    REQ_PTR(heads, "heads"); REQ_PTR(tau, "tau"); REQ_PTR(power_raw, "power_raw"); REQ_PTR(probs, "probs");
    OPT_PTR(mask, "mask"); OPT_PTR(eps, "eps"); OPT_PTR(expo, "expo"); OPT_PTR(onehot, "onehot");
    OPT_PTR(action_env, "action_env"); OPT_PTR(p_off01, "p_off01"); OPT_PTR(action_store, "action_store");
    const float fl = clamp_share_floor(cpu_share_floor);
    return finish(fn, risvec::launch_policy_sample(n_envs, n_veh, env_offset, heads, mask, tau, hard, eps, expo, seed, counter,
                                                   fl, power_raw, probs, onehot, action_env, p_off01, action_store,
                                                   (hipStream_t)stream));
}

int risvec_policy_sample_normal(int32_t n_rows, int32_t n_veh, int64_t row_offset, const float* heads, const uint8_t* mask,
                                const float* tau, const uint8_t* hard, const float* eps, const float* expo, uint64_t seed,
                                uint32_t counter, float* power, float* probs, float* next_actions, float* logp_power,
                                float* logp_intent, float* logp_power_sum, float* logp_intent_sum, risvec_stream_t stream) {
    const char* fn = "risvec_policy_sample_normal";
    if (n_rows == 0) return RISVEC_OK;                       // an empty batch: nothing to launch
    if (n_rows < 0) return fail(RISVEC_ERR_ARG, "%s: n_rows=%d must be >= 0", fn, n_rows);
    if (n_veh < 1 || n_veh > RISVEC_MAX_VEH)
        return fail(RISVEC_ERR_ARG, "%s: n_veh=%d outside [1,%d]", fn, n_veh, RISVEC_MAX_VEH);
    if (row_offset < 0 || row_offset + n_rows > 0xFFFFFFFFLL)
        return fail(RISVEC_ERR_ARG, "%s: row_offset+n_rows must fit 32 bits", fn);
    REQ_PTR(heads, "heads"); REQ_PTR(tau, "tau");
    OPT_PTR(mask, "mask"); OPT_PTR(eps, "eps"); OPT_PTR(expo, "expo");
    OPT_PTR(power, "power"); OPT_PTR(probs, "probs"); OPT_PTR(next_actions, "next_actions");
    OPT_PTR(logp_power, "logp_power"); OPT_PTR(logp_intent, "logp_intent");
    OPT_PTR(logp_power_sum, "logp_power_sum"); OPT_PTR(logp_intent_sum, "logp_intent_sum");
    if (!power && !probs && !next_actions && !logp_power && !logp_intent && !logp_power_sum && !logp_intent_sum)
        return fail(RISVEC_ERR_ARG, "%s: no output given", fn);
    if ((logp_power_sum || logp_intent_sum) && risvec::policy_sample_normal_rows_per_block(n_veh) < 1)
        return fail(RISVEC_ERR_ARG, "%s: the sums over the agents are built for n_veh <= 16 (got %d): add the per-agent "
                    "outputs instead", fn, n_veh);
    return finish(fn, risvec::launch_policy_sample_normal(n_rows, n_veh, row_offset, heads, mask, tau, hard, eps, expo, seed,
                                                          counter, power, probs, next_actions, logp_power, logp_intent,
                                                          logp_power_sum, logp_intent_sum, (hipStream_t)stream));
}

int risvec_policy_layer1(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, const float* obs, const float* W1,
                         const float* b1, const float* ln_w, const float* ln_b, float* out, risvec_stream_t stream) {
    const char* fn = "risvec_policy_layer1";
    if (n_envs < 1 || n_veh < 1 || n_veh > 65535) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d n_veh=%d", fn, n_envs, n_veh);
    if (in_dims < 1 || f1 < 1 || f1 > 1024 || (long long)(in_dims + 3) * f1 * 4 > 64 * 1024)
        return fail(RISVEC_ERR_SHAPE, "%s: in_dims=%d f1=%d (f1 <= 1024, (in+3)*f1 floats must fit 64 KB of LDS)", fn,
                    in_dims, f1);
    REQ_PTR(obs, "obs"); REQ_PTR(W1, "W1"); REQ_PTR(b1, "b1"); REQ_PTR(ln_w, "ln_w"); REQ_PTR(ln_b, "ln_b"); REQ_PTR(out, "out");
    return finish(fn, risvec::launch_policy_layer1(n_envs, n_veh, in_dims, f1, obs, W1, b1, ln_w, ln_b, out,
                                                   (hipStream_t)stream));
}

int risvec_policy_layer1_split16(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, const float* obs,
                                 const float* W1, const float* b1, const float* ln_w, const float* ln_b, void* out16,
                                 risvec_stream_t stream) {
    const char* fn = "risvec_policy_layer1_split16";
    if (n_envs < 1 || n_veh < 1 || n_veh > 65535) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d n_veh=%d", fn, n_envs, n_veh);
    if (in_dims < 1 || in_dims > 8 || f1 < 4 || f1 > 1024 || f1 % 4 != 0 || (long long)(in_dims + 3) * f1 * 4 > 64 * 1024)
        return fail(RISVEC_ERR_SHAPE, "%s: in_dims=%d f1=%d (in_dims <= 8, f1 a multiple of 4 and <= 1024)", fn, in_dims, f1);
    REQ_PTR(obs, "obs"); REQ_PTR(W1, "W1"); REQ_PTR(b1, "b1"); REQ_PTR(ln_w, "ln_w"); REQ_PTR(ln_b, "ln_b"); REQ_PTR(out16, "out16");
    return finish(fn, risvec::launch_policy_layer1_split16(n_envs, n_veh, in_dims, f1, obs, W1, b1, ln_w, ln_b, out16,
                                                           (hipStream_t)stream));
}

int risvec_policy_mlp_supported(int32_t in_dims, int32_t f1, int32_t f2, int32_t n_heads) {
    return risvec::policy_mlp_supported(in_dims, f1, f2, n_heads) ? 1 : 0;
}

int risvec_policy_mlp(int32_t n_envs, int32_t n_veh, int32_t in_dims, int32_t f1, int32_t f2, int32_t n_heads, const float* obs,
                      const float* G, const void* W1F, const void* W2f, const float* w_unscale, const float* b2,
                      const float* ln2_w, const float* ln2_b, const void* WhF, const float* wh_unscale, const float* bh,
                      float* heads, risvec_stream_t stream) {
    const char* fn = "risvec_policy_mlp";
    if (n_envs < 1 || n_veh < 1 || n_veh > 65535) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d n_veh=%d", fn, n_envs, n_veh);
    if (!risvec::policy_mlp_supported(in_dims, f1, f2, n_heads))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: in_dims=%d f1=%d f2=%d n_heads=%d (built for in_dims <= 5, f1 a multiple of 32 "
                    "and <= 1024, f2 = 128 or 256, n_heads <= 24; use risvec_policy_layer1 + a GEMM + risvec_policy_heads)", fn,
                    in_dims, f1, f2, n_heads);
    REQ_PTR(obs, "obs"); REQ_PTR(G, "G"); REQ_PTR(W1F, "W1F"); REQ_PTR(W2f, "W2f"); REQ_PTR(w_unscale, "w_unscale");
    REQ_PTR(b2, "b2"); REQ_PTR(ln2_w, "ln2_w"); REQ_PTR(ln2_b, "ln2_b"); REQ_PTR(WhF, "WhF"); REQ_PTR(wh_unscale, "wh_unscale");
    REQ_PTR(bh, "bh"); REQ_PTR(heads, "heads");
    return finish(fn, risvec::launch_policy_mlp(n_envs, n_veh, in_dims, f1, f2, n_heads, obs, G, W1F, W2f, w_unscale, b2, ln2_w,
                                                ln2_b, WhF, wh_unscale, bh, heads, (hipStream_t)stream));
}

int risvec_sarl_actor_supported(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions) {
    return risvec::sarl_actor_supported(in_dims, fc1, fc2, n_actions) ? 1 : 0;
}

int risvec_sarl_actor(int32_t n_rows, int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions, const float* x,
                      const void* wstream, int64_t wstream_bytes, const float* scales, const float* b2, const float* ln2_w,
                      const float* ln2_b, const float* bmu, float* logits, float* mu, risvec_stream_t stream) {
    const char* fn = "risvec_sarl_actor";
    if (n_rows < 1) return fail(RISVEC_ERR_SHAPE, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (!risvec::sarl_actor_supported(in_dims, fc1, fc2, n_actions))
        return fail(RISVEC_ERR_SHAPE, "%s: in_dims=%d fc1=%d fc2=%d n_actions=%d (built for in_dims <= 128, fc1 a multiple of 32 "
                    "and <= 1024, fc2 = 128 or 256, n_actions <= 96; use library kernels elsewhere)", fn, in_dims, fc1, fc2,
                    n_actions);
    const risvec::SarlActorGeom g = risvec::sarl_actor_geom(in_dims, fc1, fc2, n_actions);
    if (int rc = check_wstream_bytes(fn, "", wstream_bytes, g.stream_bytes)) return rc;
    REQ_PTR(x, "x"); REQ_PTR(wstream, "wstream"); REQ_PTR(scales, "scales"); REQ_PTR(b2, "b2"); REQ_PTR(ln2_w, "ln2_w");
    REQ_PTR(ln2_b, "ln2_b"); REQ_PTR(bmu, "bmu"); OPT_PTR(logits, "logits"); REQ_PTR(mu, "mu");
    return finish(fn, risvec::launch_sarl_actor(n_rows, in_dims, fc1, fc2, n_actions, x, wstream, scales, b2, ln2_w, ln2_b, bmu,
                                                logits, mu, (hipStream_t)stream));
}

size_t risvec_sarl_actor_pack_workspace(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions) {
    return (size_t)risvec::sarl_actor_pack_workspace(in_dims, fc1, fc2, n_actions);
}

int risvec_sarl_actor_pack(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t n_actions, const float* W1, const float* b1,
                           const float* ln1_w, const float* ln1_b, const float* W2, const float* Wmu, void* wstream,
                           size_t wstream_bytes, float* scales, void* workspace, size_t workspace_bytes,
                           risvec_stream_t stream) {
    const char* fn = "risvec_sarl_actor_pack";
    if (!risvec::sarl_actor_supported(in_dims, fc1, fc2, n_actions))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: in_dims=%d fc1=%d fc2=%d n_actions=%d (risvec_sarl_actor is built for in_dims "
                    "<= 128, fc1 a multiple of 32 and <= 1024, fc2 = 128 or 256, n_actions <= 96)", fn, in_dims, fc1, fc2,
                    n_actions);
    REQ_PTR(W1, "W1"); REQ_PTR(b1, "b1"); REQ_PTR(ln1_w, "ln1_w"); REQ_PTR(ln1_b, "ln1_b"); REQ_PTR(W2, "W2");
    REQ_PTR(Wmu, "Wmu"); REQ_PTR(wstream, "wstream"); REQ_PTR(scales, "scales"); REQ_PTR(workspace, "workspace");
    const risvec::SarlActorGeom g = risvec::sarl_actor_geom(in_dims, fc1, fc2, n_actions);
    if (int rc = check_wstream_bytes(fn, "", wstream_bytes, g.stream_bytes)) return rc;
    if (int rc = check_workspace_bytes(fn, workspace_bytes, (size_t)risvec::sarl_actor_pack_workspace(in_dims, fc1, fc2, n_actions),
                                       "shape", "risvec_sarl_actor_pack_workspace"))
        return rc;
    return finish(fn, risvec::launch_sarl_actor_pack(in_dims, fc1, fc2, n_actions, W1, b1, ln1_w, ln1_b, W2, Wmu, wstream,
                                                     scales, workspace, (hipStream_t)stream));
}

int risvec_sarl_critic_supported(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions) {
    return risvec::sarl_critic_supported(in_dims, fc1, fc2, fc3, n_actions) ? 1 : 0;
}

int64_t risvec_sarl_critic_stream_bytes(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions) {
    return risvec::sarl_critic_stream_bytes(in_dims, fc1, fc2, fc3, n_actions);
}

int risvec_sarl_critic(int32_t n_rows, int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions, const float* x,
                       const float* a, const void* wstream, int64_t wstream_bytes, const float* scales, const float* ln1_w,
                       const float* ln1_b, const float* b2, const float* ln2_w, const float* ln2_b, const float* bav,
                       const float* b3, const float* ln3_w, const float* ln3_b, const float* q_w, const float* q_b,
                       const float* reward, const uint8_t* done, float gamma, float* q_out, float* y_out,
                       risvec_stream_t stream) {
    const char* fn = "risvec_sarl_critic";
    if (n_rows < 1) return fail(RISVEC_ERR_SHAPE, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (!risvec::sarl_critic_supported(in_dims, fc1, fc2, fc3, n_actions))
        return fail(RISVEC_ERR_SHAPE, "%s: in_dims=%d fc1=%d fc2=%d fc3=%d n_actions=%d (built for in_dims <= 128, fc1 a multiple "
                    "of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or 256, n_actions <= 96; use library kernels elsewhere)",
                    fn, in_dims, fc1, fc2, fc3, n_actions);
    if (int rc = check_wstream_bytes(fn, "", wstream_bytes, risvec::sarl_critic_stream_bytes(in_dims, fc1, fc2, fc3, n_actions)))
        return rc;
    if (!x || !a) return fail(RISVEC_ERR_ARG, "%s: x or a is NULL", fn);
    REQ_PTR(wstream, "wstream"); REQ_PTR(scales, "scales"); REQ_PTR(ln1_w, "ln1_w"); REQ_PTR(ln1_b, "ln1_b"); REQ_PTR(b2, "b2");
    REQ_PTR(ln2_w, "ln2_w"); REQ_PTR(ln2_b, "ln2_b"); REQ_PTR(bav, "bav"); REQ_PTR(b3, "b3"); REQ_PTR(ln3_w, "ln3_w");
    REQ_PTR(ln3_b, "ln3_b"); REQ_PTR(q_w, "q_w");
    if (!q_b) return fail(RISVEC_ERR_ARG, "%s: q_b is NULL", fn);
    if (!q_out && !y_out) return fail(RISVEC_ERR_ARG, "%s: q_out and y_out are both NULL", fn);
    if (y_out && (!reward || !done)) return fail(RISVEC_ERR_ARG, "%s: y_out needs reward and done", fn);
    if (y_out && !std::isfinite(gamma)) return fail(RISVEC_ERR_ARG, "%s: gamma=%g must be finite", fn, (double)gamma);
    return finish(fn, risvec::launch_sarl_critic(n_rows, in_dims, fc1, fc2, fc3, n_actions, x, a, wstream, scales, ln1_w, ln1_b, b2,
                                                 ln2_w, ln2_b, bav, b3, ln3_w, ln3_b, q_w, q_b, reward, done, gamma, q_out, y_out,
                                                 (hipStream_t)stream));
}

size_t risvec_sarl_critic_pack_workspace(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions) {
    return (size_t)risvec::sarl_critic_pack_workspace(in_dims, fc1, fc2, fc3, n_actions);
}

int risvec_sarl_critic_pack(int32_t in_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_actions, const float* W1,
                            const float* b1, const float* W2, const float* Wav, const float* W3, void* wstream,
                            size_t wstream_bytes, float* scales, void* workspace, size_t workspace_bytes,
                            risvec_stream_t stream) {
    const char* fn = "risvec_sarl_critic_pack";
    if (!risvec::sarl_critic_supported(in_dims, fc1, fc2, fc3, n_actions))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: in_dims=%d fc1=%d fc2=%d fc3=%d n_actions=%d (risvec_sarl_critic is built for "
                    "in_dims <= 128, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or 256, n_actions <= 96)",
                    fn, in_dims, fc1, fc2, fc3, n_actions);
    REQ_F32_IN("", W1, "W1"); REQ_F32_IN("", b1, "b1"); REQ_F32_IN("", W2, "W2"); REQ_F32_IN("", Wav, "Wav");
    REQ_F32_IN("", W3, "W3"); REQ_F32_IN("", scales, "scales");
    REQ_PTR(wstream, "wstream"); REQ_PTR(workspace, "workspace");
    if (int rc = check_wstream_bytes(fn, "", wstream_bytes, risvec::sarl_critic_stream_bytes(in_dims, fc1, fc2, fc3, n_actions)))
        return rc;
    if (int rc = check_workspace_bytes(fn, workspace_bytes,
                                       (size_t)risvec::sarl_critic_pack_workspace(in_dims, fc1, fc2, fc3, n_actions), "shape",
                                       "risvec_sarl_critic_pack_workspace"))
        return rc;
    return finish(fn, risvec::launch_sarl_critic_pack(in_dims, fc1, fc2, fc3, n_actions, W1, b1, W2, Wav, W3, wstream, scales,
                                                      workspace, (hipStream_t)stream));
}

namespace {

// risvec_marl_critic and risvec_marl_critic_wide: one argument list, one set of checks, two rules and two kernels
int marl_critic_entry(const char* fn, bool wide, int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                      int32_t fc3, int32_t n_nets, const RisVecMarlCriticNet* nets, const float* state, const float* action,
                      const float* reward, const uint8_t* done, float gamma, const float* coef, const float* logp_power,
                      const float* logp_intent, float* q1, float* q2, float* y, risvec_stream_t stream) {
    if (n_rows < 1) return fail(RISVEC_ERR_ARG, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (n_nets < 1 || n_nets > 2) return fail(RISVEC_ERR_ARG, "%s: n_nets=%d must be 1 or 2", fn, n_nets);
    if (!(wide ? risvec::marl_critic_wide_supported : risvec::marl_critic_supported)(state_dims, action_dims, fc1, fc2, fc3))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d (built for state_dims + "
                    "action_dims <= %d, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or 256; use library "
                    "kernels elsewhere)", fn, state_dims, action_dims, fc1, fc2, fc3, wide ? 512 : 128);
    if (!nets) return fail(RISVEC_ERR_ARG, "%s: nets is NULL", fn);
    const long long bytes = (wide ? risvec::marl_critic_wide_stream_bytes : risvec::marl_critic_stream_bytes)(state_dims, action_dims,
                                                                                                              fc1, fc2, fc3);
    if (int rc = check_critic_nets(fn, nets, n_nets, bytes)) return rc;
    if (!state || !action) return fail(RISVEC_ERR_ARG, "%s: state or action is NULL", fn);
    if (int rc = check_critic_outputs(fn, n_nets, reward, done, gamma, coef, logp_power, logp_intent, q1, q2, y)) return rc;
    return finish(fn, (wide ? risvec::launch_marl_critic_wide : risvec::launch_marl_critic)(
                          n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, state, action, reward, done, gamma, coef,
                          logp_power, logp_intent, q1, q2, y, (hipStream_t)stream));
}

// risvec_marl_critic_pack and risvec_marl_critic_wide_pack, likewise; ws_fn: the entry that states the workspace
int marl_critic_pack_entry(const char* fn, const char* ws_fn, bool wide, int32_t state_dims, int32_t action_dims, int32_t fc1,
                           int32_t fc2, int32_t fc3, int32_t n_nets, const RisVecMarlCriticPackNet* nets, void* workspace,
                           size_t workspace_bytes, risvec_stream_t stream) {
    if (n_nets < 1 || n_nets > 2) return fail(RISVEC_ERR_ARG, "%s: n_nets=%d must be 1 or 2", fn, n_nets);
    if (!(wide ? risvec::marl_critic_wide_supported : risvec::marl_critic_supported)(state_dims, action_dims, fc1, fc2, fc3))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d (%s is built "
                    "for state_dims + action_dims <= %d, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or "
                    "256)", fn, state_dims, action_dims, fc1, fc2, fc3, wide ? "risvec_marl_critic_wide" : "risvec_marl_critic",
                    wide ? 512 : 128);
    if (!nets) return fail(RISVEC_ERR_ARG, "%s: nets is NULL", fn);
    const long long bytes = (wide ? risvec::marl_critic_wide_stream_bytes : risvec::marl_critic_stream_bytes)(state_dims, action_dims,
                                                                                                              fc1, fc2, fc3);
    for (int c = 0; c < n_nets; ++c) {
        const RisVecMarlCriticPackNet& n = nets[c];
        const Indexed pre("nets", c);
        REQ_F32_IN(pre.s, n.W1, "W1"); REQ_F32_IN(pre.s, n.W2, "W2"); REQ_F32_IN(pre.s, n.W3, "W3");
        REQ_F32_IN(pre.s, n.scales, "scales");
        REQ_PTR_IN(pre.s, n.wstream, "wstream");
        if (int rc = check_wstream_bytes(fn, pre.s, n.wstream_bytes, bytes)) return rc;
    }
    if (n_nets == 2 && nets[0].wstream == nets[1].wstream)
        return fail(RISVEC_ERR_ARG, "%s: nets[0].wstream and nets[1].wstream are the same buffer", fn);
    if (n_nets == 2 && nets[0].scales == nets[1].scales)
        return fail(RISVEC_ERR_ARG, "%s: nets[0].scales and nets[1].scales are the same buffer", fn);
    REQ_PTR(workspace, "workspace");
    const long long need = (wide ? risvec::marl_critic_wide_pack_workspace : risvec::marl_critic_pack_workspace)(
        state_dims, action_dims, fc1, fc2, fc3, n_nets);
    if (int rc = check_workspace_bytes(fn, workspace_bytes, (size_t)need, "call", ws_fn)) return rc;
    return finish(fn, (wide ? risvec::launch_marl_critic_wide_pack : risvec::launch_marl_critic_pack)(
                          state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, workspace, (hipStream_t)stream));
}

}  // namespace

int risvec_marl_critic_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_supported(state_dims, action_dims, fc1, fc2, fc3) ? 1 : 0;
}

int64_t risvec_marl_critic_stream_bytes(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_stream_bytes(state_dims, action_dims, fc1, fc2, fc3);
}

int risvec_marl_critic(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                       int32_t n_nets, const RisVecMarlCriticNet* nets, const float* state, const float* action,
                       const float* reward, const uint8_t* done, float gamma, const float* coef, const float* logp_power,
                       const float* logp_intent, float* q1, float* q2, float* y, risvec_stream_t stream) {
    return marl_critic_entry("risvec_marl_critic", false, n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, state, action,
                             reward, done, gamma, coef, logp_power, logp_intent, q1, q2, y, stream);
}

size_t risvec_marl_critic_pack_workspace(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                                         int32_t n_nets) {
    return (size_t)risvec::marl_critic_pack_workspace(state_dims, action_dims, fc1, fc2, fc3, n_nets);
}

int risvec_marl_critic_pack(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_nets,
                            const RisVecMarlCriticPackNet* nets, void* workspace, size_t workspace_bytes,
                            risvec_stream_t stream) {
    return marl_critic_pack_entry("risvec_marl_critic_pack", "risvec_marl_critic_pack_workspace", false, state_dims, action_dims, fc1,
                                  fc2, fc3, n_nets, nets, workspace, workspace_bytes, stream);
}

int risvec_marl_critic_wide_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_wide_supported(state_dims, action_dims, fc1, fc2, fc3) ? 1 : 0;
}

int64_t risvec_marl_critic_wide_stream_bytes(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_wide_stream_bytes(state_dims, action_dims, fc1, fc2, fc3);
}

int risvec_marl_critic_wide(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                            int32_t n_nets, const RisVecMarlCriticNet* nets, const float* state, const float* action,
                            const float* reward, const uint8_t* done, float gamma, const float* coef, const float* logp_power,
                            const float* logp_intent, float* q1, float* q2, float* y, risvec_stream_t stream) {
    return marl_critic_entry("risvec_marl_critic_wide", true, n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, state,
                             action, reward, done, gamma, coef, logp_power, logp_intent, q1, q2, y, stream);
}

size_t risvec_marl_critic_wide_pack_workspace(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                                              int32_t n_nets) {
    return (size_t)risvec::marl_critic_wide_pack_workspace(state_dims, action_dims, fc1, fc2, fc3, n_nets);
}

int risvec_marl_critic_wide_pack(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3, int32_t n_nets,
                                 const RisVecMarlCriticPackNet* nets, void* workspace, size_t workspace_bytes,
                                 risvec_stream_t stream) {
    return marl_critic_pack_entry("risvec_marl_critic_wide_pack", "risvec_marl_critic_wide_pack_workspace", true, state_dims,
                                  action_dims, fc1, fc2, fc3, n_nets, nets, workspace, workspace_bytes, stream);
}

int risvec_marl_critic_grad_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_grad_supported(state_dims, action_dims, fc1, fc2, fc3) ? 1 : 0;
}

size_t risvec_marl_critic_grad_workspace(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                         int32_t fc3, int32_t n_nets) {
    return risvec::marl_critic_grad_workspace(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets);
}

int risvec_marl_critic_grad(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3,
                            int32_t n_nets, const RisVecMarlCriticGradNet* nets, const RisVecMarlCriticGrads* grads,
                            const float* state, const float* action, const float* target, float* q1, float* q2, float* loss,
                            void* workspace, size_t workspace_bytes, risvec_stream_t stream) {
    const char* fn = "risvec_marl_critic_grad";
    if (n_rows < 1) return fail(RISVEC_ERR_ARG, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (n_nets < 1 || n_nets > 2) return fail(RISVEC_ERR_ARG, "%s: n_nets=%d must be 1 or 2", fn, n_nets);
    if (!risvec::marl_critic_grad_supported(state_dims, action_dims, fc1, fc2, fc3))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d (built for state_dims + "
                    "action_dims <= 128, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or 256; use library "
                    "kernels elsewhere)", fn, state_dims, action_dims, fc1, fc2, fc3);
    if (!nets) return fail(RISVEC_ERR_ARG, "%s: nets is NULL", fn);
    if (!grads) return fail(RISVEC_ERR_ARG, "%s: grads is NULL", fn);
    const long long bytes = risvec::marl_critic_stream_bytes(state_dims, action_dims, fc1, fc2, fc3);
    for (int c = 0; c < n_nets; ++c) {
        const RisVecMarlCriticNet& n = nets[c].fwd;
        const Indexed pre("nets", c);
        if (int rc = check_wstream_bytes(fn, pre.s, n.wstream_bytes, bytes)) return rc;
        REQ_PTR_IN(pre.s, n.wstream, "wstream"); REQ_PTR_IN(pre.s, n.scales, "scales"); REQ_PTR_IN(pre.s, n.b1, "b1");
        REQ_PTR_IN(pre.s, n.b2, "b2"); REQ_PTR_IN(pre.s, n.b3, "b3"); REQ_PTR_IN(pre.s, n.qw, "qw");
        if (!n.qb) return fail(RISVEC_ERR_ARG, "%s: %sqb is NULL", fn, pre.s);
        REQ_F32_IN(pre.s, nets[c].W2, "W2"); REQ_F32_IN(pre.s, nets[c].W3, "W3");
        const RisVecMarlCriticGrads& g = grads[c];
        const Indexed gpre("grads", c);
        REQ_F32_IN(gpre.s, g.dW1, "dW1"); REQ_F32_IN(gpre.s, g.db1, "db1"); REQ_F32_IN(gpre.s, g.dW2, "dW2");
        REQ_F32_IN(gpre.s, g.db2, "db2"); REQ_F32_IN(gpre.s, g.dW3, "dW3"); REQ_F32_IN(gpre.s, g.db3, "db3");
        REQ_F32_IN(gpre.s, g.dqw, "dqw"); REQ_F32_IN(gpre.s, g.dqb, "dqb");
    }
    {   // one writer per gradient tensor
        const float* all[16];
        int k = 0;
        for (int c = 0; c < n_nets; ++c) {
            const RisVecMarlCriticGrads& g = grads[c];
            for (const float* p : {g.dW1, g.db1, g.dW2, g.db2, g.dW3, g.db3, g.dqw, g.dqb}) all[k++] = p;
        }
        for (int a = 0; a < k; ++a)
            for (int b = a + 1; b < k; ++b)
                if (all[a] == all[b]) return fail(RISVEC_ERR_ARG, "%s: two gradient tensors are the same buffer", fn);
    }
    if (!state || !action) return fail(RISVEC_ERR_ARG, "%s: state or action is NULL", fn);
    OPT_F32_IN("", state, "state"); OPT_F32_IN("", action, "action");
    REQ_F32_IN("", target, "target");
    REQ_F32_IN("", q1, "q1");
    if (n_nets == 2) REQ_F32_IN("", q2, "q2");
    else if (q2) return fail(RISVEC_ERR_ARG, "%s: q2 needs n_nets == 2", fn);
    if (n_nets == 2 && q1 == q2) return fail(RISVEC_ERR_ARG, "%s: q1 and q2 are the same buffer", fn);
    REQ_F32_IN("", loss, "loss");
    REQ_PTR(workspace, "workspace");
    const size_t need = risvec::marl_critic_grad_workspace(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets);
    if (int rc = check_workspace_bytes(fn, workspace_bytes, need, "call", "risvec_marl_critic_grad_workspace")) return rc;
    return finish(fn, risvec::launch_marl_critic_grad(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, grads, state, action,
                                                      target, q1, q2, loss, workspace, (hipStream_t)stream));
}

int risvec_marl_critic_action_grad_supported(int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2, int32_t fc3) {
    return risvec::marl_critic_action_grad_supported(state_dims, action_dims, fc1, fc2, fc3) ? 1 : 0;
}

size_t risvec_marl_critic_action_grad_workspace(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1,
                                                int32_t fc2, int32_t fc3, int32_t n_nets) {
    return risvec::marl_critic_action_grad_workspace(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets);
}

int risvec_marl_critic_action_grad(int32_t n_rows, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                   int32_t fc3, int32_t n_nets, const RisVecMarlCriticActionGradNet* nets, const float* state,
                                   const float* action, float scale, float* q1, float* q2, float* q_min, float* out,
                                   void* workspace, size_t workspace_bytes, risvec_stream_t stream) {
    const char* fn = "risvec_marl_critic_action_grad";
    if (n_rows < 1) return fail(RISVEC_ERR_ARG, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (n_nets < 1 || n_nets > 2) return fail(RISVEC_ERR_ARG, "%s: n_nets=%d must be 1 or 2", fn, n_nets);
    if (!risvec::marl_critic_action_grad_supported(state_dims, action_dims, fc1, fc2, fc3))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d (built for state_dims + "
                    "action_dims <= 128, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, fc3 = 128 or 256; use library "
                    "kernels elsewhere)", fn, state_dims, action_dims, fc1, fc2, fc3);
    if (!nets) return fail(RISVEC_ERR_ARG, "%s: nets is NULL", fn);
    const long long bytes = risvec::marl_critic_stream_bytes(state_dims, action_dims, fc1, fc2, fc3);
    for (int c = 0; c < n_nets; ++c) {
        const RisVecMarlCriticNet& n = nets[c].fwd;
        const Indexed pre("nets", c);
        if (int rc = check_wstream_bytes(fn, pre.s, n.wstream_bytes, bytes)) return rc;
        REQ_PTR_IN(pre.s, n.wstream, "wstream"); REQ_PTR_IN(pre.s, n.scales, "scales"); REQ_PTR_IN(pre.s, n.b1, "b1");
        REQ_PTR_IN(pre.s, n.b2, "b2"); REQ_PTR_IN(pre.s, n.b3, "b3"); REQ_PTR_IN(pre.s, n.qw, "qw");
        if (!n.qb) return fail(RISVEC_ERR_ARG, "%s: %sqb is NULL", fn, pre.s);
        REQ_F32_IN(pre.s, nets[c].W1, "W1"); REQ_F32_IN(pre.s, nets[c].W2, "W2"); REQ_F32_IN(pre.s, nets[c].W3, "W3");
    }
    if (!state || !action) return fail(RISVEC_ERR_ARG, "%s: state or action is NULL", fn);
    OPT_F32_IN("", state, "state"); OPT_F32_IN("", action, "action");
    if (!std::isfinite(scale)) return fail(RISVEC_ERR_ARG, "%s: scale must be finite", fn);
    OPT_F32_IN("", q1, "q1"); OPT_F32_IN("", q2, "q2"); OPT_F32_IN("", q_min, "q_min");
    if (n_nets == 1 && q2) return fail(RISVEC_ERR_ARG, "%s: q2 needs n_nets == 2", fn);
    if (q1 && q1 == q2) return fail(RISVEC_ERR_ARG, "%s: q1 and q2 are the same buffer", fn);
    REQ_F32_IN("", out, "out");
    REQ_PTR(workspace, "workspace");
    const size_t need = risvec::marl_critic_action_grad_workspace(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets);
    if (int rc = check_workspace_bytes(fn, workspace_bytes, need, "call", "risvec_marl_critic_action_grad_workspace")) return rc;
    return finish(fn, risvec::launch_marl_critic_action_grad(n_rows, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, state, action,
                                                             scale, q1, q2, q_min, out, workspace, (hipStream_t)stream));
}

int risvec_local_critics_supported(int32_t n_agents, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                                   int32_t fc3) {
    return risvec::local_critics_supported(n_agents, state_dims, action_dims, fc1, fc2, fc3) ? 1 : 0;
}

int risvec_local_critics(int32_t n_rows, int32_t n_agents, int32_t state_dims, int32_t action_dims, int32_t fc1, int32_t fc2,
                         int32_t fc3, int32_t n_nets, const RisVecMarlCriticNet* nets, const float* obs, const float* action,
                         const float* heads, const float* power, const float* reward, const uint8_t* done, float gamma,
                         const float* coef, const float* logp_power, const float* logp_intent, float* q1, float* q2, float* y,
                         risvec_stream_t stream) {
    const char* fn = "risvec_local_critics";
    if (n_rows < 1) return fail(RISVEC_ERR_ARG, "%s: n_rows=%d must be >= 1", fn, n_rows);
    if (n_nets < 1 || n_nets > 2) return fail(RISVEC_ERR_ARG, "%s: n_nets=%d must be 1 or 2", fn, n_nets);
    if (!risvec::local_critics_supported(n_agents, state_dims, action_dims, fc1, fc2, fc3))
        return fail(RISVEC_ERR_UNSUPPORTED, "%s: n_agents=%d state_dims=%d action_dims=%d fc1=%d fc2=%d fc3=%d (built for 1 <= "
                    "n_agents <= %d, state_dims + action_dims <= 128, fc1 a multiple of 32 and <= 1024, fc2 = 128, 256 or 512, "
                    "fc3 = 128 or 256; use library kernels elsewhere)", fn, n_agents, state_dims, action_dims, fc1, fc2, fc3,
                    risvec::kLocalCriticsMaxAgents);
    if (!nets) return fail(RISVEC_ERR_ARG, "%s: nets is NULL", fn);
    if (int rc = check_critic_nets(fn, nets, n_agents * n_nets,
                                   risvec::marl_critic_stream_bytes(state_dims, action_dims, fc1, fc2, fc3)))
        return rc;
    if (!obs) return fail(RISVEC_ERR_ARG, "%s: obs is NULL", fn);
    if (action && heads) return fail(RISVEC_ERR_ARG, "%s: action and heads are both given (one of them builds the input)", fn);
    if (!action && !heads) return fail(RISVEC_ERR_ARG, "%s: action and heads are both NULL", fn);
    if (heads && !power) return fail(RISVEC_ERR_ARG, "%s: heads needs power", fn);
    if (power && !heads) return fail(RISVEC_ERR_ARG, "%s: power needs heads", fn);
    if (heads && action_dims != n_agents + 2)
        return fail(RISVEC_ERR_ARG, "%s: heads needs action_dims == n_agents + 2, got action_dims=%d n_agents=%d", fn, action_dims,
                    n_agents);
    if (int rc = check_critic_outputs(fn, n_nets, reward, done, gamma, coef, logp_power, logp_intent, q1, q2, y)) return rc;
    return finish(fn, risvec::launch_local_critics(n_rows, n_agents, state_dims, action_dims, fc1, fc2, fc3, n_nets, nets, obs,
                                                   action, heads, power, reward, done, gamma, coef, logp_power, logp_intent, q1,
                                                   q2, y, (hipStream_t)stream));
}

int risvec_soft_update(int32_t n_tensors, const float* const* online, float* const* target, const int64_t* numel, float tau,
                       float one_minus_tau, risvec_stream_t stream) {
    const char* fn = "risvec_soft_update";
    if (n_tensors < 1 || n_tensors > risvec::kSoftUpdateMax)
        return fail(RISVEC_ERR_SHAPE, "%s: n_tensors=%d outside [1, %d]", fn, n_tensors, risvec::kSoftUpdateMax);
    if (!online || !target || !numel) return fail(RISVEC_ERR_ARG, "%s: online, target or numel is NULL", fn);
    if (!std::isfinite(tau) || !std::isfinite(one_minus_tau))
        return fail(RISVEC_ERR_ARG, "%s: tau=%g and one_minus_tau=%g must be finite", fn, (double)tau, (double)one_minus_tau);
    long long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 1 || numel[i] > (1LL << 40))
            return fail(RISVEC_ERR_SHAPE, "%s: numel[%d]=%lld outside [1, 2^40]", fn, i, (long long)numel[i]);
        if (!online[i] || !target[i]) return fail(RISVEC_ERR_ARG, "%s: online[%d] or target[%d] is NULL", fn, i, i);
        if ((reinterpret_cast<uintptr_t>(online[i]) | reinterpret_cast<uintptr_t>(target[i])) & 3u)
            return fail(RISVEC_ERR_ARG, "%s: online[%d] or target[%d] is not 4-byte aligned", fn, i, i);
        if (online[i] == target[i])
            return fail(RISVEC_ERR_ARG, "%s: online[%d] and target[%d] are the same tensor", fn, i, i);
        total += numel[i];
    }
    if (total > (1LL << 40)) return fail(RISVEC_ERR_SHAPE, "%s: %lld elements in all, more than 2^40", fn, total);
    return finish(fn, risvec::launch_soft_update(n_tensors, online, target, numel, tau, one_minus_tau, (hipStream_t)stream));
}

size_t risvec_adam_workspace(int32_t n_blocks) { return n_blocks < 1 ? 0 : (size_t)n_blocks * sizeof(double); }

int risvec_adam_step(int32_t n_tensors, int32_t n_groups, int32_t n_blocks, const RisVecAdamTensor* tensors,
                     const RisVecAdamGroup* groups, const int32_t* block_tensor, const RisVecAdamTensor* tensors_host,
                     const RisVecAdamGroup* groups_host, double beta1, double beta2, double eps, int64_t t, float tau,
                     float one_minus_tau, uint32_t flags, double* partials, size_t partials_bytes, float* norms,
                     risvec_stream_t stream) {
    const char* fn = "risvec_adam_step";
    static_assert(sizeof(RisVecAdamTensor) == 64 && sizeof(RisVecAdamGroup) == 32, "descriptor layout");
    if (n_tensors < 1 || n_tensors > (1 << 20))
        return fail(RISVEC_ERR_SHAPE, "%s: n_tensors=%d outside [1, 2^20]", fn, n_tensors);
    if (n_groups < 1 || n_groups > n_tensors)
        return fail(RISVEC_ERR_SHAPE, "%s: n_groups=%d outside [1, n_tensors=%d]", fn, n_groups, n_tensors);
    if (n_blocks < n_tensors) return fail(RISVEC_ERR_SHAPE, "%s: n_blocks=%d is below n_tensors=%d", fn, n_blocks, n_tensors);
    REQ_PTR(tensors, "tensors"); REQ_PTR(groups, "groups"); REQ_PTR(block_tensor, "block_tensor");
    if (!tensors_host) return fail(RISVEC_ERR_ARG, "%s: tensors_host is NULL", fn);
    if (!groups_host) return fail(RISVEC_ERR_ARG, "%s: groups_host is NULL", fn);
    if (flags & ~(uint32_t)(RISVEC_ADAM_CLIP | RISVEC_ADAM_WRITE_GRAD | RISVEC_ADAM_BLEND))
        return fail(RISVEC_ERR_ARG, "%s: flags 0x%x: only CLIP / WRITE_GRAD / BLEND are accepted", fn, flags);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(RISVEC_ERR_ARG, "%s: beta1=%g outside [0, 1)", fn, beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(RISVEC_ERR_ARG, "%s: beta2=%g outside [0, 1)", fn, beta2);
    if (!std::isfinite(eps) || eps < 0.0) return fail(RISVEC_ERR_ARG, "%s: eps=%g must be finite and >= 0", fn, eps);
    if (t < 1) return fail(RISVEC_ERR_ARG, "%s: t=%lld must be >= 1", fn, (long long)t);
    const bool blend = (flags & RISVEC_ADAM_BLEND) != 0, clip = (flags & RISVEC_ADAM_CLIP) != 0;
    if (blend && (!std::isfinite(tau) || !std::isfinite(one_minus_tau)))
        return fail(RISVEC_ERR_ARG, "%s: tau=%g and one_minus_tau=%g must be finite", fn, (double)tau, (double)one_minus_tau);
    int group = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const RisVecAdamTensor& d = tensors_host[i];
        if (d.numel < 1 || d.numel > (1LL << 40))
            return fail(RISVEC_ERR_SHAPE, "%s: tensors[%d].numel=%lld outside [1, 2^40]", fn, i, (long long)d.numel);
        if ((d.group != group && d.group != group + 1) || (i == 0 && d.group != 0) || d.group >= n_groups)
            return fail(RISVEC_ERR_ARG, "%s: tensors[%d].group=%d (tensors are listed group by group from 0, none empty, "
                        "n_groups=%d)", fn, i, d.group, n_groups);
        group = d.group;
    }
    if (group != n_groups - 1) return fail(RISVEC_ERR_ARG, "%s: %d groups have tensors, n_groups=%d", fn, group + 1, n_groups);
    long long blocks = 0;
    group = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const RisVecAdamTensor& d = tensors_host[i];
        const bool opens = i == 0 || d.group != group;
        group = d.group;
        if (opens && groups_host[group].first_block != blocks)
            return fail(RISVEC_ERR_ARG, "%s: groups[%d].first_block=%d, its tensors start at workgroup %lld", fn, group,
                        groups_host[group].first_block, blocks);
        if (d.first_block != blocks)
            return fail(RISVEC_ERR_ARG, "%s: tensors[%d].first_block=%d, the numels before it give %lld", fn, i, d.first_block,
                        blocks);
        const struct { const float* p; const char* name; } ptrs[] = {{d.param, "param"}, {d.grad, "grad"}, {d.exp_avg, "exp_avg"},
                                                                     {d.exp_avg_sq, "exp_avg_sq"}, {d.target, "target"}};
        const Indexed pre("tensors", i);
        for (int k = 0; k < 5; ++k) {
            if (k < 4) REQ_F32_IN(pre.s, ptrs[k].p, ptrs[k].name);
            else OPT_F32_IN(pre.s, ptrs[k].p, ptrs[k].name);      // target: NULL where the tensor has none
            for (int j = 0; j < k; ++j)
                if (ptrs[k].p && ptrs[k].p == ptrs[j].p)
                    return fail(RISVEC_ERR_ARG, "%s: tensors[%d].%s and .%s are the same tensor", fn, i, ptrs[j].name, ptrs[k].name);
        }
        blocks += (d.numel + RISVEC_ADAM_CHUNK - 1) / RISVEC_ADAM_CHUNK;
        if (blocks > 0x7fffffffLL) return fail(RISVEC_ERR_SHAPE, "%s: more than 2^31 - 1 workgroups", fn);
        const bool closes = i + 1 == n_tensors || tensors_host[i + 1].group != group;
        if (closes && groups_host[group].n_blocks != blocks - groups_host[group].first_block)
            return fail(RISVEC_ERR_ARG, "%s: groups[%d].n_blocks=%d, its tensors take %lld workgroups", fn, group,
                        groups_host[group].n_blocks, blocks - groups_host[group].first_block);
    }
    if (blocks != n_blocks) return fail(RISVEC_ERR_SHAPE, "%s: n_blocks=%d, the numels give %lld", fn, n_blocks, blocks);
    for (int g = 0; g < n_groups; ++g) {
        const RisVecAdamGroup& G = groups_host[g];
        if (!std::isfinite(G.lr) || G.lr < 0.0) return fail(RISVEC_ERR_ARG, "%s: groups[%d].lr=%g must be finite and >= 0", fn, g, G.lr);
        if (!std::isfinite(G.weight_decay) || G.weight_decay < 0.f)
            return fail(RISVEC_ERR_ARG, "%s: groups[%d].weight_decay=%g must be finite and >= 0", fn, g, (double)G.weight_decay);
        if (std::isnan(G.max_norm)) return fail(RISVEC_ERR_ARG, "%s: groups[%d].max_norm is NaN (< 0 disables clipping)", fn, g);
    }
    if (clip) {
        REQ_PTR(partials, "partials");
        REQ_F32_IN("", norms, "norms");
        if (partials_bytes < risvec_adam_workspace(n_blocks))
            return fail(RISVEC_ERR_ARG, "%s: partials_bytes=%zu, this call needs %zu (risvec_adam_workspace)", fn, partials_bytes,
                        risvec_adam_workspace(n_blocks));
    }
    risvec::AdamLaunch a{};
    a.tensors = tensors; a.groups = groups; a.block_tensor = block_tensor; a.partials = partials; a.norms = norms;
    a.bc1 = 1.0 - std::pow(beta1, (double)t);                 // torch/optim/adam.py: 1 - beta1 ** step, in double
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)t));
    a.omb1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.tau = tau; a.omt = one_minus_tau;
    a.n_tensors = n_tensors; a.n_groups = n_groups; a.n_blocks = n_blocks; a.flags = flags;
    return finish(fn, risvec::launch_adam_step(a, (hipStream_t)stream));
}

int risvec_policy_heads(int32_t n_envs, int32_t n_veh, int32_t f2, int32_t n_heads, const float* g, const float* b2,
                        const float* ln_w, const float* ln_b, const float* Wh, const float* bh, float* heads,
                        risvec_stream_t stream) {
    const char* fn = "risvec_policy_heads";
    if (n_envs < 1 || n_veh < 1 || n_veh > 65535) return fail(RISVEC_ERR_SHAPE, "%s: n_envs=%d n_veh=%d", fn, n_envs, n_veh);
    if (f2 < 1 || f2 > 1024 || n_heads < 1 || ((long long)3 * f2 + (long long)f2 * n_heads + n_heads) * 4 > 64 * 1024)
        return fail(RISVEC_ERR_SHAPE, "%s: f2=%d n_heads=%d (f2 <= 1024, f2*(n_heads+2) floats must fit 64 KB of LDS)", fn,
                    f2, n_heads);
    REQ_PTR(g, "g"); OPT_PTR(b2, "b2"); REQ_PTR(ln_w, "ln_w"); REQ_PTR(ln_b, "ln_b"); REQ_PTR(Wh, "Wh"); REQ_PTR(bh, "bh");
    REQ_PTR(heads, "heads");
    return finish(fn, risvec::launch_policy_heads(n_envs, n_veh, f2, n_heads, g, b2, ln_w, ln_b, Wh, bh, heads,
                                                  (hipStream_t)stream));
}

static int episode_dims(const char* fn, int32_t n_envs, int32_t n_veh) {
    if (int rc = check_envs_veh(fn, n_envs, n_veh)) return rc;
    if ((long long)n_envs * (RISVEC_EP_FIXED + n_veh) >= (1LL << 31))
        return fail(RISVEC_ERR_SHAPE, "%s: n_envs*(%d+n_veh) must stay below 2^31", fn, RISVEC_EP_FIXED);
    return RISVEC_OK;
}

int risvec_episode_clear(int32_t n_envs, int32_t n_veh, double* acc, risvec_stream_t stream) {
    const char* fn = "risvec_episode_clear";
    if (int rc = episode_dims(fn, n_envs, n_veh)) return rc;
    REQ_PTR(acc, "acc");
    return finish(fn, risvec::launch_episode_clear(n_envs, n_veh, acc, (hipStream_t)stream));
}

int risvec_episode_accumulate(int32_t n_envs, int32_t n_veh, const float* metrics, const float* reward,
                              const float* power_w, float user_clip, double* acc, risvec_stream_t stream) {
    const char* fn = "risvec_episode_accumulate";
    if (int rc = episode_dims(fn, n_envs, n_veh)) return rc;
    REQ_PTR(metrics, "metrics"); REQ_PTR(reward, "reward"); OPT_PTR(power_w, "power_w"); REQ_PTR(acc, "acc");
    if (!(user_clip >= 0.0f)) return fail(RISVEC_ERR_ARG, "%s: user_clip=%g must be >= 0", fn, (double)user_clip);
    return finish(fn, risvec::launch_episode_accumulate(n_envs, n_veh, metrics, reward, power_w, user_clip, acc,
                                                        (hipStream_t)stream));
}

int32_t risvec_episode_partial_rows(int32_t n_envs) { return n_envs < 1 ? 0 : risvec::episode_partial_rows(n_envs); }

int risvec_episode_summary(int32_t n_envs, int32_t n_veh, int32_t n_steps, const double* acc, const float* metrics,
                           double* per_env, double* partial, double* summary, risvec_stream_t stream) {
    const char* fn = "risvec_episode_summary";
    if (int rc = episode_dims(fn, n_envs, n_veh)) return rc;
    if (n_steps < 1) return fail(RISVEC_ERR_ARG, "%s: n_steps=%d must be >= 1 (no step was accumulated)", fn, n_steps);
    REQ_PTR(acc, "acc"); REQ_PTR(metrics, "metrics"); OPT_PTR(per_env, "per_env"); REQ_PTR(partial, "partial");
    REQ_PTR(summary, "summary");
    return finish(fn, risvec::launch_episode_summary(n_envs, n_veh, n_steps, acc, metrics, per_env, partial, summary,
                                                     (hipStream_t)stream));
}

}  // extern "C"
