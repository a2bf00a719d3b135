// The fused step under a 3GPP channel model (phy.channel_model 3gpp_umi / 3gpp_uma / other): update_channel_gains
// (ENV:255-327, the RIS ignored: path loss x log-normal shadow x Rayleigh / Rice power from the vehicle's position) and
// step() (ENV:547-731) in ONE launch.
//
// Layout of k_step<VP> (k_step.hip): one lane per (env, vehicle), the V lanes of an env in an aligned group of
// VP = pow2_ceil(V) lanes.  A lane requests its position (16 bytes) and its draws with the step inputs, computes the
// gain in registers through the same device function as k_gain_3gpp (risvec_3gpp.hpp), stores it to state.gain and
// runs step_core -- the two-launch form k_gain_3gpp + k_step bit for bit, without the gain's round trip through HBM
// and the second launch.  Neither h_r nor theta is read: every V <= 64 and every M is served.
//   k_step_3gpp<VP>          one step
//   k_step_3gpp<VP,RING>     + the replay transition store (RingIn / ring_store as k_step<VP,RING>), V in {4, 8, 16}
//   k_step_3gpp<VP,MULTI>    T steps; fresh fading (chan_counter + t) and arrivals (counter + t) every step, the
//                            position-only half of the gain (distances, p_LOS, both path losses) hoisted out of the loop
#include "risvec_3gpp.hpp"
#include "risvec_step.hpp"

namespace risvec {

enum Form3gpp { kPlain3gpp = 0, kRing3gpp = 1, kMulti3gpp = 2 };

// the draws of lane idx: injected (slice `off` of the [T,]E,V arrays) or Philox at `counter`
__device__ __forceinline__ Draws3gpp lane_draws_3gpp(const Dims& d, const RisVecParams& P, const StepArgs& A,
                                                     const Chan3gpp& C, int e, int v, long long off, uint32_t counter) {
    Draws3gpp r;
    if (C.u_los) {
        r.u = C.u_los[off]; r.z = C.z_shadow[off]; r.sm = C.small[off];
    } else {
        r = draws_3gpp(P.rician_k_db, (uint32_t)(d.env_offset + e), (uint32_t)v, counter, A.seed);
    }
    return r;
}

// gain of step t of the T-step launch, from the hoisted position-only terms; keeps the last value (state.gain)
struct Gain3gppSteps {
    const Dims& d;
    const RisVecParams& P;
    const StepArgs& A;
    const Chan3gpp& C;
    int e, v;
    bool active;
    long long idx, ev;
    double p_los, large_los, large_nlos;
    float last;
    __device__ __forceinline__ float operator()(int t) {
        float g = 0.f;
        if (active) {
            const Draws3gpp r = lane_draws_3gpp(d, P, A, C, e, v, idx + (long long)t * ev, C.chan_counter + (uint32_t)t);
            const bool los = r.u < p_los;
            g = gain_3gpp_draw(P, los ? large_los : large_nlos, los, r);
        }
        last = g;
        return g;
    }
};

template <int VP, int FORM>
__global__ void __launch_bounds__(kBlock)
k_step_3gpp(Dims d, RisVecParams P, StepArgs A, Chan3gpp C, int n_steps, RisVecTraj TJ) {
    RISVEC_ARGS_IN_ONE_TRIP("s"(d.E), "s"(d.V), "s"(A.flags), "s"(A.action), "s"(A.data_buf), "s"(A.partner), "s"(A.n_groups),
                            "s"(A.mec_q), "s"(A.gain), "s"(A.pl), "s"(A.arrivals), "s"(C.pos), "s"(C.u_los));
    RISVEC_ARGS_IN_ONE_TRIP(RISVEC_STEP_PARAMS(P));
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(t / VP), v = (int)(t % VP);
    const bool active = e < d.E && v < d.V;
    const long long idx = (long long)e * d.V + v;
    double2 xy = make_double2(0.0, 0.0);
    if (active) xy = reinterpret_cast<const double2*>(C.pos)[idx];          // with the step inputs
    const StepIn in = load_step_in(d, A, e, v, active);
    if constexpr (FORM == kMulti3gpp) {
        Gain3gppSteps gs{d, P, A, C, e, v, active, idx, (long long)d.E * d.V, 0.0, 0.0, 0.0, 0.f};
        if (active) {
            const Geo3gpp geo = geo_3gpp(P, xy.x, xy.y);
            gs.p_los = p_los_3gpp(geo);
            gs.large_los = large_3gpp(P, C.model, true, geo);
            gs.large_nlos = large_3gpp(P, C.model, false, geo);
        }
        multi_step_loop<VP>(d, P, A, TJ, e, v, active, &gs, in, n_steps);
        if (active) A.gain[idx] = gs.last;
    } else {
        float g = 0.f;
        if (active) {
            const Draws3gpp r = lane_draws_3gpp(d, P, A, C, e, v, idx, C.chan_counter);
            g = gain_3gpp(P, C.model, xy.x, xy.y, r);
            A.gain[idx] = g;
        }
        if constexpr (FORM == kRing3gpp) {
            const RingIn<VP> rin = load_ring_in<VP>(d, A, e, v, active);
            step_core<VP, false, true, RingIn<VP>>(d, P, A, e, v, active, g, in, nullptr, &rin);
        } else {
            step_core<VP, false, true>(d, P, A, e, v, active, g, in);
        }
    }
}

template <int VP>
static hipError_t launch_step_3gpp_vp(const RisVecState& s, const RisVecParams& p, const StepArgs& a, const Chan3gpp& c,
                                      const StepPlan& pl, int n_steps, const RisVecTraj& tj, hipStream_t st) {
    const long long threads = (long long)s.n_envs * VP;
    const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock)), block(kBlock);
    const Dims d = dims_of(s);
    if (pl.multi) {
        hipLaunchKernelGGL((k_step_3gpp<VP, kMulti3gpp>), grid, block, 0, st, d, p, a, c, n_steps, tj);
        return hipGetLastError();
    }
    if (pl.ring) {
        if constexpr (VP == 4 || VP == 8 || VP == 16) {
            hipLaunchKernelGGL((k_step_3gpp<VP, kRing3gpp>), grid, block, 0, st, d, p, a, c, 1, tj);
            return hipGetLastError();
        }
        return hipErrorNotSupported;
    }
    hipLaunchKernelGGL((k_step_3gpp<VP, kPlain3gpp>), grid, block, 0, st, d, p, a, c, 1, tj);
    return hipGetLastError();
}

hipError_t launch_step_3gpp(const RisVecState& s, const RisVecParams& p, const StepArgs& a, const Chan3gpp& c, int form,
                            int n_steps, const RisVecTraj& tj, hipStream_t st) {
    const StepPlan pl = plan_step(s, RISVEC_STEP_3GPP, form);
    if (pl.family != StepPlan::G3) return hipErrorNotSupported;
    const hipError_t err =
        with_vp(s.n_veh, [&](auto vp) { return launch_step_3gpp_vp<vp>(s, p, a, c, pl, n_steps, tj, st); });
    note_kernel("%s", pl.name);
    return err;
}

}  // namespace risvec
