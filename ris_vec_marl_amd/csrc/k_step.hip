// The hot path, generic shapes: RIS cascaded gain (K3), step() (K4) and their fusion
// (K34) for ANY (V <= 64, M); compile-time shapes take the software-pipelined kernels of
// k_step_pipe.hip instead.
//
// Reference: Simulation-MARL-BCD/Environment.py (ENV): update_channel_gains "free"
// ENV:263-273, compute_data_rate ENV:331-372, step ENV:547-731.
//
// Work decomposition (wave64, no MFMA: this is a bandwidth-bound reduction path):
//   * cascade: a group of G lanes (G = 8..64, power of two) owns one (env, vehicle)
//     row h_r[e,v,:], reads it with 16-byte loads (two complex per lane), multiplies
//     by w = theta[e,:] * b[:] and reduces the complex partial sums over the group
//     with wavefront shuffles.
//   * step: one lane per (env, vehicle); the V lanes of an env sit in an aligned group
//     of VP = pow2ceil(V) lanes, so the four cross-vehicle couplings of step() (NOMA
//     partner gain/power, sum of edge cycles, the V-means) are group shuffles.
//   * fused: a wave owns 64/VP consecutive envs; it streams their h_r rows, parks the
//     reduced sums in its private LDS slice, then every lane picks up "its" (env,
//     vehicle) sum and runs the step.  One HBM pass over h_r/theta, gains never
//     round-trip through HBM before use.
#include <type_traits>

#include "risvec_pipe.hpp"

namespace risvec {

// K3: standalone gain kernel, one G-lane group per (env, vehicle)
template <int G, int VEC>
__global__ void __launch_bounds__(kBlock)
k_gain(Dims d, const float* __restrict__ h_r, const float* __restrict__ theta,
       const float* __restrict__ b, const float* __restrict__ pl, const float* __restrict__ h_d,
       float* __restrict__ gain) {
    constexpr int UPB = kBlock / G;                       // (env,veh) units per block
    const int gl = threadIdx.x % G;
    const long long u = (long long)blockIdx.x * UPB + threadIdx.x / G;
    const bool valid = u < (long long)d.E * d.V;
    const long long uu = valid ? u : 0;
    const long long e = uu / d.V;
    const float2 img = cascade_row<G, VEC>(h_r + uu * d.M * 2, theta + e * d.M * 2, b, d.M, gl, valid);
    if (valid && gl == 0) gain[u] = gain_from_img(img, pl[u], h_d, u);
}

// K4: standalone step kernel (cached gains; the reference's per-step cadence)
// RING: the env's replay transition is written from here too (StepArgs::ring; marl_train_bcd.py:1776-1799)
template <int VP, bool RING = false>
__global__ void __launch_bounds__(kBlock)
k_step(Dims d, RisVecParams P, StepArgs A) {
    RISVEC_ARGS_IN_ONE_TRIP("s"(d.E), "s"(d.V), "s"(A.flags), "s"(A.action), "s"(A.data_buf), "s"(A.partner), "s"(A.n_groups),
                            "s"(A.mec_q), "s"(A.gain), "s"(A.pl), "s"(A.arrivals));
    RISVEC_ARGS_IN_ONE_TRIP(RISVEC_STEP_PARAMS(P));
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(t / VP), v = (int)(t % VP);
    const bool active = e < d.E && v < d.V;
    const StepIn in = load_step_in(d, A, e, v, active);
    const float g = active ? A.gain[(long long)e * d.V + v] : 0.f;
    if constexpr (RING) {
        const RingIn<VP> rin = load_ring_in<VP>(d, A, e, v, active);
        step_core<VP, false, true, RingIn<VP>>(d, P, A, e, v, active, g, in, nullptr, &rin);
    } else {
        step_core<VP, false, true>(d, P, A, e, v, active, g, in);
    }
}

// K4 over T steps: the driver's own cadence (marl_train_bcd.py:1304-1611: step() every step, the channel gains only every
// K_STEPS_FOR_RIS_OPTIMIZATION = 100 steps) in ONE launch -- n_steps consecutive step() calls on the cached gains, for
// any shape.  A lane owns one (env, vehicle) for the whole launch; the env's queues stay in registers, every step's
// records go to their slice of the trajectory buffers, the env's own tensors receive the last step's outputs:
// bit-identical to n_steps launches of k_step.
template <int VP>
__global__ void __launch_bounds__(kBlock)
k_step_multi(Dims d, RisVecParams P, StepArgs A, int n_steps, RisVecTraj TJ) {
    RISVEC_ARGS_IN_ONE_TRIP("s"(d.E), "s"(d.V), "s"(A.flags), "s"(A.action), "s"(A.data_buf), "s"(A.partner), "s"(A.n_groups),
                            "s"(A.mec_q), "s"(A.gain), "s"(A.pl), "s"(A.arrivals), "s"(n_steps));
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(t / VP), v = (int)(t % VP);
    const bool active = e < d.E && v < d.V;
    const StepIn in = load_step_in(d, A, e, v, active);
    const float g = active ? A.gain[(long long)e * d.V + v] : 0.f;
    multi_step_loop<VP>(d, P, A, TJ, e, v, active, g, in, n_steps);
}

// compute_data_rate as its own entry point (ENV:331-372)
template <int VP>
__global__ void __launch_bounds__(kBlock)
k_data_rate(Dims d, RisVecParams P, const float* __restrict__ p_off, const float* __restrict__ gain,
            const int32_t* __restrict__ partner, const int32_t* __restrict__ n_groups,
            float* __restrict__ rate_out) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(t / VP), v = (int)(t % VP);
    const bool active = e < d.E && v < d.V;
    const long long idx = (long long)e * d.V + v;
    const float g = active ? gain[idx] : 0.f;
    const float pw = active ? p_off[idx] : 0.f;
    const int part = active ? partner[idx] : RISVEC_PARTNER_NONE;
    const int G = active ? n_groups[e] : 1;
    const float r = noma_rate<VP>(P, pw, g, part, G);
    if (active) rate_out[idx] = r;
}

// K34, generic: fused gain + step.  Each wave owns 64/VP consecutive envs.
template <int VP, int G, int VEC>
__global__ void __launch_bounds__(kBlock)
k_step_fused(Dims d, RisVecParams P, StepArgs A) {
    constexpr int EPW = kWave / VP;                        // envs per wave
    constexpr int VPP = kWave / G;                         // vehicles per pass
    __shared__ float2 s_img[kBlock / kWave][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gl = lane % G, gv = lane / G;
    const int e0 = (blockIdx.x * (kBlock / kWave) + wave) * EPW;
    const int V = d.V, M = d.M;

    const int e_mine = e0 + lane / VP, v_mine = lane % VP;
    const bool active = e_mine < d.E && v_mine < V;
    const StepIn in = load_step_in(d, A, e_mine, v_mine, active);   // issued ahead of the cascade

    for (int i = 0; i < EPW; ++i) {
        const int e = e0 + i;                              // wave-uniform
        if (e >= d.E) break;
        const float* trow = A.theta + (long long)e * M * 2;
        for (int v0 = 0; v0 < V; v0 += VPP) {
            const int v = v0 + gv;
            const bool valid = v < V;
            const float* hrow = A.h_r + ((long long)e * V + (valid ? v : 0)) * M * 2;
            const float2 img = cascade_row<G, VEC>(hrow, trow, A.b, M, gl, valid);
            if (valid && gl == 0) s_img[wave][i * VP + v] = img;
        }
    }
    __syncthreads();

    float g = 0.f;
    if (active) {
        const long long idx = (long long)e_mine * V + v_mine;
        g = gain_from_img(s_img[wave][lane], in.pl, A.h_d, idx);
        A.gain[idx] = g;
    }
    step_core<VP>(d, P, A, e_mine, v_mine, active, g, in);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// "Steering" form of the fused kernel (RISVEC_STEP_STEER).  compute_parms makes every row of h_r a
// geometric sequence, h_r[e,v,m] = z^m with z = exp(-j pi angle_v) (ENV:249-253), so the cascade
// sum_m theta_m b_m h_r[e,v,m] is the polynomial sum_m w_m z^m, w = theta * b.  Instead of streaming the
// 8M-byte row from HBM, a lane reads its 16-byte z (float64) and evaluates the polynomial by Horner's
// rule in float64 -- four interleaved chains in z^4, so the dependent chain is M/4 long -- against the
// env's w row staged once per wavefront in LDS.  Accumulated error ~M * 2^-53: better than the float32
// sum over the stored float32 row.  Per env-step the kernel moves 16V + 8M + 64V + 68 bytes instead of
// 8VM + 8M + 64V + 68 (1 220 vs 5 188 at V = 8, M = 64).
// WIDE: the staged w row is widened to float64 once (saves two conversions per Horner step) when 4
// wavefronts' worth of it still leaves room for several blocks per CU; long rows stay float32 in LDS.
template <int VP, bool WIDE>
__global__ void __launch_bounds__(kBlock)
k_step_steer(Dims d, RisVecParams P, StepArgs A, const double* __restrict__ z_r) {
    constexpr int EPW = kWave / VP;                        // envs per wave
    using W2 = typename std::conditional<WIDE, double2, float2>::type;
    extern __shared__ double2 s_wrow_raw[];                // [waves][EPW][M + 1]   w = theta * b (padded rows)
    W2* s_wrow = reinterpret_cast<W2*>(s_wrow_raw);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int V = d.V, M = d.M, MS = M + 1;
    const int e0 = (blockIdx.x * (blockDim.x / kWave) + wave) * EPW;
    W2* sw = s_wrow + (long long)wave * EPW * MS;
    const int e_mine = e0 + lane / VP, v_mine = lane % VP;
    const bool active = e_mine < d.E && v_mine < V;
    const StepIn in = load_step_in(d, A, e_mine, v_mine, active);
    double2 z = make_double2(1.0, 0.0);
    if (active) z = reinterpret_cast<const double2*>(z_r)[(long long)e_mine * V + v_mine];
    for (int idx = lane; idx < EPW * M; idx += kWave) {   // coalesced theta rows of the wave's envs
        const int i = idx / M, m = idx - i * M;
        const int e = e0 + i;
        float2 w = make_float2(0.f, 0.f);
        if (e < d.E) {
            const float2 t = *reinterpret_cast<const float2*>(A.theta + ((long long)e * M + m) * 2);
            w = cmul(t, *reinterpret_cast<const float2*>(A.b + m * 2));
        }
        if constexpr (WIDE) sw[i * MS + m] = make_double2((double)w.x, (double)w.y);
        else sw[i * MS + m] = w;
    }
    __syncthreads();
    // z^2, z^4 and four Horner chains over m = 4k + r, highest power first
    const double z2r = z.x * z.x - z.y * z.y, z2i = 2.0 * z.x * z.y;
    const double z4r = z2r * z2r - z2i * z2i, z4i = 2.0 * z2r * z2i;
    const W2* wr = sw + (lane / VP) * MS;
    double ar[4] = {0.0, 0.0, 0.0, 0.0}, ai[4] = {0.0, 0.0, 0.0, 0.0};
    const int M4 = (M + 3) / 4;
    for (int k = M4 - 1; k >= 0; --k) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * k + r;
            double wx = 0.0, wy = 0.0;
            if (m < M) { const W2 w = wr[m]; wx = (double)w.x; wy = (double)w.y; }
            const double nr = ar[r] * z4r - ai[r] * z4i + wx;
            const double ni = ar[r] * z4i + ai[r] * z4r + wy;
            ar[r] = nr; ai[r] = ni;
        }
    }
    // sum_r z^r acc_r = acc0 + z (acc1 + z (acc2 + z acc3))
    double sr = ar[3], si = ai[3];
#pragma unroll
    for (int r = 2; r >= 0; --r) {
        const double nr = sr * z.x - si * z.y + ar[r], ni = sr * z.y + si * z.x + ai[r];
        sr = nr; si = ni;
    }
    float g = 0.f;
    if (active) {
        const long long idx = (long long)e_mine * V + v_mine;
        g = gain_from_img(make_float2((float)sr, (float)si), in.pl, A.h_d, idx);
        A.gain[idx] = g;
    }
    step_core<VP>(d, P, A, e_mine, v_mine, active, g, in);
}

// LDS of the steering kernel per wavefront: its EPW envs' rows of M + 1 w values, float64 ("wide") when 4 wavefronts' worth
// still leave room for several blocks per CU, float32 for long rows
static size_t steer_lds_per_wave(int vp, int n_ris, bool* wide) {
    const size_t row = (size_t)(kWave / vp) * (n_ris + 1);
    *wide = row * sizeof(double2) * (kBlock / kWave) <= 40 * 1024;     // >= 4 blocks per CU either way
    return row * (*wide ? sizeof(double2) : sizeof(float2));
}

template <int VP>
static hipError_t launch_steer_vp(const RisVecState& s, const RisVecParams& p, const StepArgs& a, hipStream_t st) {
    constexpr int EPW = kWave / VP;
    bool wide;
    const size_t per_wave = steer_lds_per_wave(VP, s.n_ris, &wide);
    int waves = (int)((64 * 1024) / per_wave);             // as many wavefronts per block as 64 KB of LDS hold (>= 1: plan_step)
    if (waves > kBlock / kWave) waves = kBlock / kWave;
    const long long n_waves = ((long long)s.n_envs + EPW - 1) / EPW;
    const dim3 grid((unsigned)((n_waves + waves - 1) / waves)), block(waves * kWave);
    if (wide) hipLaunchKernelGGL((k_step_steer<VP, true>), grid, block, per_wave * waves, st, dims_of(s), p, a, s.z_r);
    else hipLaunchKernelGGL((k_step_steer<VP, false>), grid, block, per_wave * waves, st, dims_of(s), p, a, s.z_r);
    return hipGetLastError();
}

template <int G>
static hipError_t launch_gain_g(const RisVecState& s, hipStream_t st) {
    const long long units = (long long)s.n_envs * s.n_veh;
    const unsigned grid = (unsigned)((units + (kBlock / G) - 1) / (kBlock / G));
    if ((s.n_ris & 1) == 0)
        hipLaunchKernelGGL((k_gain<G, 2>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), s.h_r, s.theta,
                           s.b, s.pl, s.h_d, s.gain);
    else
        hipLaunchKernelGGL((k_gain<G, 1>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), s.h_r, s.theta,
                           s.b, s.pl, s.h_d, s.gain);
    return hipGetLastError();
}

hipError_t launch_gain(const RisVecState& s, const RisVecParams&, hipStream_t st) {
    {
        const hipError_t err = launch_gain_pipe(s, st);     // compile-time shapes: pipelined form
        if (err != hipErrorNotSupported) return err;
    }
    const int vec = (s.n_ris & 1) ? 1 : 2;
    switch (pick_group(s.n_ris, vec, kWave)) {
        case 8: return launch_gain_g<8>(s, st);
        case 16: return launch_gain_g<16>(s, st);
        case 32: return launch_gain_g<32>(s, st);
        default: return launch_gain_g<64>(s, st);
    }
}

// the generic members: cached k_step<VP> (RING: with the transition store), fused k_step_fused<VP,G,VEC>, k_step_steer<VP>
template <int VP>
static hipError_t launch_step_vp(const RisVecState& s, const RisVecParams& p, const StepArgs& a, const StepPlan& pl,
                                 hipStream_t st) {
    const long long threads = (long long)s.n_envs * VP;
    const unsigned grid = (unsigned)((threads + kBlock - 1) / kBlock);
    const Dims d = dims_of(s);
    if (pl.family == StepPlan::STEER) return launch_steer_vp<VP>(s, p, a, st);
    if (pl.family == StepPlan::CACHED) {
        if constexpr (VP == 4 || VP == 8 || VP == 16) {
            if (pl.ring) {
                hipLaunchKernelGGL((k_step<VP, true>), dim3(grid), dim3(kBlock), 0, st, d, p, a);
                return hipGetLastError();
            }
        }
        hipLaunchKernelGGL((k_step<VP>), dim3(grid), dim3(kBlock), 0, st, d, p, a);
        return hipGetLastError();
    }
#define RISVEC_FUSED(GG)                                                                          \
    if (pl.g == GG) {                                                                             \
        if (pl.vec == 2) hipLaunchKernelGGL((k_step_fused<VP, GG, 2>), dim3(grid), dim3(kBlock), 0, st, d, p, a); \
        else hipLaunchKernelGGL((k_step_fused<VP, GG, 1>), dim3(grid), dim3(kBlock), 0, st, d, p, a);             \
        return hipGetLastError();                                                                 \
    }
    if constexpr (kWave / VP <= 8) { RISVEC_FUSED(8) }
    if constexpr (kWave / VP <= 16) { RISVEC_FUSED(16) }
    if constexpr (kWave / VP <= 32) { RISVEC_FUSED(32) }
    RISVEC_FUSED(64)
#undef RISVEC_FUSED
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// The selector: which member of the step family a call launches.  Every dispatch rule of the family lives here, in the
// order it applies (DESIGN.md 3.1 points here).  stream = h_r + theta bytes of one step = E (8VM + 8M); IC = the
// Infinity Cache; the thresholds are tuning()'s (risvec_pipe.hpp: 256 CUs and 256 MiB on MI355X).
//
//   RISVEC_STEP_3GPP (risvec_step_fused_3gpp*; reads neither h_r nor theta, so any V <= 64 and any M):
//     fused                 k_step_3gpp<VP>
//     fused + ring          k_step_3gpp<VP,RING>, V in {4, 8, 16}
//     fused T-step          k_step_3gpp<VP,MULTI>
//     (no cached forms: the cached step does not depend on the channel model)
//   cached (risvec_step)    k_step<VP>, VP = pow2_ceil(V)
//   cached + ring           k_step<VP,RING>, V in {4, 8, 16}
//   fused + ring            the compile-time shapes' pipeline k_step_fused_pipe<V,M,D,MarlCore+ring> (NT as in 4.)
//   fused T-step            the compile-time shapes with V <= 8: k_step_fused_lat<V,M,EPWT,MULTI>
//   fused, the first that applies:
//     1. RISVEC_STEP_THETA_BY_INDEX   k_step_fused_lat<..,EMAX,TK> (NT / ALT by stream size as in 3.)
//     2. RISVEC_STEP_STEER            k_step_steer<VP,wide|narrow> while one wavefront's theta rows fit 64 KB of LDS
//     3. V in {4, 8, 16}, even M <= 256: the latency-shaped k_step_fused_lat (k_step_lat.hip)
//          stream > 1.29 IC           EMAX envs per wavefront, NT
//          IC < stream <= 1.29 IC     EMAX, ALT
//          otherwise                  EPWT envs per wavefront, while 8x64 and 4x16 have at most 24 wavefronts (of 4
//                                     envs) per CU and 16x64 at most 8 (16x64: never NT); 8x36, 8x40, 16x256 and the
//                                     run-time-M members at every size
//     4. the compile-time shapes      k_step_fused_pipe<V,M,D,MarlCore> (NT beyond 1.055 IC)
//     5. anything else                k_step_fused<VP,G,VEC>
//   RISVEC_STEP_THETA_IDX_CURRENT selects nothing -- no plan and no name changes.  Where the plan is byte-bound and has a
//   by-index instantiation, launch_step hands it state.theta_idx and that instantiation reads theta as 1-byte indices:
//     the pipeline of 4. and its ring form, with or without NT      k_step_fused_pipe<..,NT?,TK>
//     the NT and ALT members of 3. (always EMAX envs per wavefront) k_step_fused_lat<..,EMAX,NT|ALT,TK>
//   Everywhere else the bit is ignored: the default-policy members of 3. (one memory round trip, not byte-bound: a table
//   fill in front of their first use for nothing), the steering, generic and 3GPP kernels.
//   RISVEC_STEP_H_R_STEER_CURRENT selects nothing either.  Where the plan is the pipeline of 4. or its ring form (either
//   cache policy), M % 16 == 0 and the state carries steer_ang and z_r, launch_step runs the pipeline's GEN member
//   k_step_fused_gen<V,M,Core,TK?> (k_step_gen.hip): the rows are rebuilt by steer_chunk(), not read; the walk is the
//   pipeline's (the order of a wavefront's groups).  Everywhere else the bit is ignored.
//   RISVEC_STEP_STEER_HEADS_CURRENT rides on that bit: where the GEN member runs, its HD form reads the chunk heads
//   kept behind state.steer_ang (risvec_steer_heads) instead of evaluating them; where it does not, the bit is dropped.
//
// Why (us per step; profiles/):
//   * beyond 1.29 IC many short wavefronts with every request up front are what the best pure reader looks like: 1-4 %
//     faster than the pipeline's long-lived wavefronts (r02t_lat_nt_experiment.txt, pipeline / this: 65 536 envs
//     59.3 / 58.5, 131 072 115.8 / 111.9, 262 144 223.6 / 217.1; with the default cache policy it loses 7-12 % there);
//   * in (1, 1.29] IC the default policy with the envs walked in alternating directions from step to step is 3-12 %
//     faster than the hint (r03q_pingpong_band.txt);
//   * the crossover at 8 x 64 (r02t_lat_vs_pipe.txt, this / pipeline: 8 192 envs 7.3 / 9.4, 12 288 11.5 / 12.5,
//     20 480 17.9 / 18.7, 24 576 21.2 / 21.1, 32 768 27.5 / 26.9); at 16 x 64 (r02t_lat_v16.txt, pipeline / this:
//     4 096 envs 8.0 / 7.0, 8 192 14.5 / 14.5, from 16 384 the pipeline wins); M = 36 / 40 at every size
//     (r02u_lat_vs_pipe_ragged.txt); 16 x 256, one env per wavefront (r02t_lat_v16.txt: 2 048 envs 14.6 -> 13.5,
//     4 096 25.3 -> 23.4; BASELINE configs[4] with the BCD sweep 251.5 -> 233);
//   * EPWT = the largest of {4, 2, 1} that keeps >= 8 wavefronts per CU (r02t_lat_epw_sweep.txt), clamped to the
//     member's [EMIN, EMAX];
//   * the T-step loop is instruction-issue-bound (~400 dependent-ish vector instructions per step and wavefront whatever
//     the number of active lanes): EPWT = 64 / V envs per wavefront (at most 8), halved while fewer than 4 wavefronts
//     per CU.
// risvec_force_forms() (tests and same-box A/Bs only) overrides the lat / pipeline choice, the envs per wavefront and the
// cache policies.
// ---------------------------------------------------------------------------
namespace {

struct Fixed { int V, M, D, emin, emax; bool tstep; };
constexpr Fixed kFixed[] = {
#define RISVEC_X(V_, M_, D_, EMIN, EMAX, T) {V_, M_, D_, EMIN, EMAX, T},
    RISVEC_FIXED_SHAPES(RISVEC_X)
#undef RISVEC_X
};
struct RuntimeM { int V, G, NIT, emin, emax; };
constexpr RuntimeM kRuntimeM[] = {
#define RISVEC_X(V_, G_, NIT_, EMIN, EMAX) {V_, G_, NIT_, EMIN, EMAX},
    RISVEC_RUNTIME_M_SHAPES(RISVEC_X)
#undef RISVEC_X
};

const Fixed* fixed_shape(int V, int M) {
    for (const Fixed& f : kFixed)
        if (f.V == V && f.M == M) return &f;
    return nullptr;
}

long long stream_bytes(const RisVecState& s) { return (long long)s.n_envs * (8LL * s.n_veh * s.n_ris + 8LL * s.n_ris); }

// M = 0: the run-time-M member (G, NIT) at s.n_ris
StepPlan lat_plan(const RisVecState& s, int M, int G, int NIT, int epwt, int pol, bool tk, bool multi) {
    StepPlan pl;
    pl.family = StepPlan::LAT;
    pl.V = s.n_veh; pl.M = M; pl.G = G; pl.NIT = NIT;
    pl.epwt = epwt; pl.pol = pol; pl.tk = tk; pl.multi = multi;
    const char* ps = pol == 1 ? ",NT" : (pol == 2 ? ",ALT" : "");
    if (M)
        snprintf(pl.name, sizeof(pl.name), "k_step_fused_lat<%d,%d,%d%s%s%s>", pl.V, M, epwt, multi ? ",MULTI" : "", ps,
                 tk ? ",TK" : "");
    else
        snprintf(pl.name, sizeof(pl.name), "k_step_fused_lat<%d,M=%d(G=%d,NIT=%d),%d%s%s%s>", pl.V, s.n_ris, G, NIT, epwt,
                 multi ? ",MULTI" : "", ps, tk ? ",TK" : "");
    return pl;
}

// rules 1 and 3
StepPlan plan_lat(const RisVecState& s, bool tk) {
    const int V = s.n_veh, M = s.n_ris;
    if (!step_fused_lat_covers(V, M)) return {};
    const RisVecForce& F = forced_forms();
    const Tuning& T = tuning();
    const long long b = stream_bytes(s);
    const bool off = F.lat == RISVEC_FORCE_OFF;
    bool nt = !off && forced_or(F.lat_nt, b > T.lat_nt_from);
    const bool walk = forced_or(F.lat_alt, b > T.ic_bytes && b <= T.lat_nt_from);
    const bool band = !off && !nt && walk && b > T.ic_bytes;
    // wavefronts (of 4 envs) per CU up to which this kernel beats the shape's software pipeline
    auto below = [&](int waves_per_cu) {
        return F.lat == RISVEC_FORCE_ON || (!off && s.n_envs <= (long long)waves_per_cu * T.cus * 4);
    };
    const Fixed* f = fixed_shape(V, M);
    if ((V == 8 && M == 64) || (V == 4 && M == 16)) {
        if (!nt && !band && !tk && !below(24)) return {};
    } else if (V == 16 && M == 64) {
        if (!below(8) && !tk) return {};
        nt = false;
    } else if (f && off && !tk) {
        return {};
    }
    int emin, emax, G = 0, NIT = 0;
    if (f) {
        emin = f->emin; emax = f->emax;
    } else {
        const RuntimeM* r = nullptr;
        for (const RuntimeM& x : kRuntimeM)
            if (x.V == V && x.G == fused_g(V, M) && x.NIT == fused_nit(V, M)) r = &x;
        if (!r) return {};
        emin = r->emin; emax = r->emax; G = r->G; NIT = r->NIT;
    }
    const int pol = nt ? 1 : (walk ? 2 : 0);
    if (tk || pol) return lat_plan(s, f ? M : 0, G, NIT, emax, pol, tk, false);     // these forms: the EMAX member only
    int epwt = F.lat_epw;
    if (!epwt) {
        epwt = 4;
        while (epwt > 1 && (long long)s.n_envs / epwt < 8LL * T.cus) epwt >>= 1;
    }
    epwt = epwt < emin ? emin : (epwt > emax ? emax : epwt);
    return lat_plan(s, f ? M : 0, G, NIT, epwt, 0, false, false);
}

StepPlan plan_tstep(const RisVecState& s) {
    const Fixed* f = fixed_shape(s.n_veh, s.n_ris);
    if (!f || !f->tstep) return {};
    int epwt = kWave / pow2_ceil(s.n_veh);
    if (epwt > 8) epwt = 8;
    while (epwt > 1 && (long long)s.n_envs / epwt < 4LL * tuning().cus) epwt >>= 1;
    return lat_plan(s, f->M, 0, 0, epwt, 0, false, true);
}

StepPlan plan_steer(const RisVecState& s) {
    StepPlan pl;
    bool wide;
    if ((64 * 1024) / steer_lds_per_wave(pow2_ceil(s.n_veh), s.n_ris, &wide) < 1) return pl;   // rows too long for LDS
    pl.family = StepPlan::STEER;
    pl.vp = pow2_ceil(s.n_veh);
    snprintf(pl.name, sizeof(pl.name), "k_step_steer<%d,%s>", pl.vp, wide ? "wide" : "narrow");
    return pl;
}

// the 3GPP members (k_step_3gpp.hip): one per form, any shape
StepPlan plan_3gpp(const RisVecState& s, int form) {
    StepPlan pl;
    const int V = s.n_veh;
    if (form == RISVEC_FORM_FUSED_RING && V != 4 && V != 8 && V != 16) return pl;
    if (form != RISVEC_FORM_FUSED && form != RISVEC_FORM_FUSED_RING && form != RISVEC_FORM_FUSED_MULTI) return pl;
    pl.family = StepPlan::G3;
    pl.vp = pow2_ceil(V);
    pl.ring = form == RISVEC_FORM_FUSED_RING;
    pl.multi = form == RISVEC_FORM_FUSED_MULTI;
    snprintf(pl.name, sizeof(pl.name), "k_step_3gpp<%d%s>", pl.vp, pl.ring ? ",RING" : (pl.multi ? ",MULTI" : ""));
    return pl;
}

StepPlan plan_generic(const RisVecState& s, bool fused, bool ring) {
    StepPlan pl;
    pl.vp = pow2_ceil(s.n_veh);
    if (fused) {
        pl.family = StepPlan::FUSED;
        pl.vec = (s.n_ris & 1) ? 1 : 2;
        pl.g = pick_group(s.n_ris, pl.vec, pl.vp);
        snprintf(pl.name, sizeof(pl.name), "k_step_fused<%d,%d,%d>", pl.vp, pl.g, pl.vec);
    } else if (!ring || pl.vp == 4 || pl.vp == 8 || pl.vp == 16) {
        pl.family = StepPlan::CACHED;
        pl.ring = ring;
        snprintf(pl.name, sizeof(pl.name), ring ? "k_step<%d,RING>" : "k_step<%d>", pl.vp);
    }
    return pl;
}

}  // namespace

StepPlan plan_pipe(const RisVecState& s, const char* core) {
    StepPlan pl;
    const Fixed* f = fixed_shape(s.n_veh, s.n_ris);
    if (!f) return pl;
    pl.family = StepPlan::PIPE;
    pl.V = f->V; pl.M = f->M;
    pl.pol = forced_or(forced_forms().pipe_nt, stream_bytes(s) > tuning().pipe_nt_from) ? 1 : 0;
    snprintf(pl.name, sizeof(pl.name), "k_step_fused_pipe<%d,%d,%d,%s%s>", f->V, f->M, f->D, core, pl.pol ? ",NT" : "");
    return pl;
}

StepPlan plan_step(const RisVecState& s, uint32_t flags, int form) {
    if (flags & RISVEC_STEP_3GPP) return plan_3gpp(s, form);
    switch (form) {
        case RISVEC_FORM_CACHED: return plan_generic(s, false, false);
        case RISVEC_FORM_CACHED_RING: return plan_generic(s, false, true);
        case RISVEC_FORM_FUSED_RING: {
            StepPlan pl = plan_pipe(s, MarlRingCore<8>::name());    // (one name for every V)
            pl.ring = true;
            return pl;
        }
        case RISVEC_FORM_FUSED_MULTI: return plan_tstep(s);
        case RISVEC_FORM_FUSED: break;
        default: return {};
    }
    if (flags & RISVEC_STEP_THETA_BY_INDEX) return plan_lat(s, true);
    if (flags & RISVEC_STEP_STEER) {
        const StepPlan pl = plan_steer(s);
        if (pl.family != StepPlan::NONE) return pl;
    }
    const StepPlan lat = plan_lat(s, false);
    if (lat.family != StepPlan::NONE) return lat;
    const StepPlan pipe = plan_pipe(s, MarlCore::name());
    if (pipe.family != StepPlan::NONE) return pipe;
    return plan_generic(s, true, false);
}

hipError_t launch_step(const RisVecState& s, const RisVecParams& p, const float* action,
                       const int32_t* partner, const int32_t* n_groups, const int32_t* arrivals,
                       uint64_t seed, uint32_t counter, uint32_t flags, bool fused, hipStream_t st, const StepRing* ring) {
    const int form = fused ? (ring ? RISVEC_FORM_FUSED_RING : RISVEC_FORM_FUSED) : (ring ? RISVEC_FORM_CACHED_RING : RISVEC_FORM_CACHED);
    const StepPlan pl = plan_step(s, flags, form);
    if (pl.family == StepPlan::NONE) return hipErrorNotSupported;
    StepArgs a = make_step_args(s, action, partner, n_groups, arrivals, seed, counter,
                                flags & ~(uint32_t)(RISVEC_STEP_STEER | RISVEC_STEP_THETA_BY_INDEX | RISVEC_STEP_THETA_IDX_CURRENT |
                                                    RISVEC_STEP_H_R_STEER_CURRENT | RISVEC_STEP_STEER_HEADS_CURRENT));
    if (ring) a.ring = *ring;                                  // the transition store rides in the step kernel
    // theta is kept by index (the API checked the shape), or the indices are known to match the tensor and the plan is one
    // of the byte-bound kernels with a by-index instantiation: the software pipeline (either cache policy, the ring form
    // included), or the latency family's EMAX member with the non-temporal hint or the alternating walk.  Not the latency
    // members with the default policy: they live for one memory round trip, and a table fill in front of their first use
    // would buy nothing.
    const bool idx_current = (flags & RISVEC_STEP_THETA_IDX_CURRENT) &&
                             (pl.family == StepPlan::PIPE || (pl.family == StepPlan::LAT && pl.pol != 0));
    if (pl.tk || idx_current) {
        a.theta_k = s.theta_idx;
        a.theta_k_stride = theta_idx_stride(s.n_ris);
    }
    // h_r is known to be what risvec_geometry wrote from steer_ang / z_r, and the plan is the software pipeline at a shape
    // whose rows are whole 16-element chunks: its GEN member rebuilds the rows instead of reading them (same bits).
    const bool gen = (flags & RISVEC_STEP_H_R_STEER_CURRENT) && pl.family == StepPlan::PIPE && pl.M % 16 == 0 &&
                     s.steer_ang != nullptr && s.z_r != nullptr;
    // ... and the chunk heads stand behind the angles: the member that reads them instead of evaluating sincospi (the
    // same float64 pair either way).  No plan and no name changes; dropped wherever the GEN member is.  (A GEN shape has
    // V in {4, 8, 16}, so the heads, n_envs * n_veh doubles behind a 16-byte aligned pointer, are 16-byte aligned.)
    const bool heads = gen && (flags & RISVEC_STEP_STEER_HEADS_CURRENT);
    hipError_t err;
    if (pl.family == StepPlan::LAT) err = launch_step_fused_lat(s, p, a, pl, 1, RisVecTraj{}, st);
    else if (pl.family == StepPlan::PIPE) {
        // The pipeline with the default cache policy walks the envs forward on even steps and backward on odd ones (the
        // parity ALT uses): a launch then starts on the lines the launch before read last (EXPERIMENTS.md 2026-10-19).  Same kernel
        // name, same results; RisVecForce::pipe_rev pins the direction.  The GEN member keeps the walk (the order of a
        // wavefront's groups) for what it still reads.
        const bool rev = pl.pol == 0 && forced_or(forced_forms().pipe_rev, (a.counter & 1u) != 0);
        err = gen ? launch_step_fused_gen(s, p, a, pl, rev, heads, st) : launch_step_fused_pipe(s, p, a, pl, rev, st);
    }
    else err = with_vp(s.n_veh, [&](auto vp) { return launch_step_vp<vp>(s, p, a, pl, st); });
    note_kernel("%s", pl.name);
    note_theta_by_index(a.theta_k != nullptr);
    note_h_r_rebuilt(gen);
    note_h_r_heads(heads);
    return err;
}

hipError_t launch_step_fused_multi(const RisVecState& s, const RisVecParams& p, const StepArgs& a, int n_steps,
                                   const RisVecTraj* traj, hipStream_t st) {
    const StepPlan pl = plan_step(s, 0, RISVEC_FORM_FUSED_MULTI);
    if (pl.family == StepPlan::NONE) return hipErrorNotSupported;
    const hipError_t err = launch_step_fused_lat(s, p, a, pl, n_steps, traj ? *traj : RisVecTraj{}, st);
    note_kernel("%s", pl.name);
    return err;
}

template <int VP>
static hipError_t launch_step_multi_vp(const RisVecState& s, const RisVecParams& p, const StepArgs& a, int n_steps,
                                       const RisVecTraj& tj, hipStream_t st) {
    const long long threads = (long long)s.n_envs * VP;
    const unsigned grid = (unsigned)((threads + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_step_multi<VP>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), p, a, n_steps, tj);
    note_kernel("k_step_multi<%d>", VP);
    return hipGetLastError();
}

hipError_t launch_step_multi(const RisVecState& s, const RisVecParams& p, const StepArgs& a, int n_steps,
                             const RisVecTraj* traj, hipStream_t st) {
    const RisVecTraj tj = traj ? *traj : RisVecTraj{nullptr, nullptr, nullptr};
    return with_vp(s.n_veh, [&](auto vp) { return launch_step_multi_vp<vp>(s, p, a, n_steps, tj, st); });
}

template <int VP>
static hipError_t launch_rate_vp(const RisVecState& s, const RisVecParams& p, const float* p_off,
                                 const int32_t* partner, const int32_t* n_groups, float* rate_out,
                                 hipStream_t st) {
    const long long threads = (long long)s.n_envs * VP;
    const unsigned grid = (unsigned)((threads + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_data_rate<VP>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), p, p_off, s.gain,
                       partner, n_groups, rate_out);
    return hipGetLastError();
}

hipError_t launch_data_rate(const RisVecState& s, const RisVecParams& p, const float* p_off,
                            const int32_t* partner, const int32_t* n_groups, float* rate_out,
                            hipStream_t st) {
    return with_vp(s.n_veh, [&](auto vp) { return launch_rate_vp<vp>(s, p, p_off, partner, n_groups, rate_out, st); });
}

}  // namespace risvec
