// f1: the SARL rollout step in ONE launch -- everything Simulation-SARL/ddpg_train.py:114-185 does between
// the actor's output and the replay buffer, per env with A = 2V + M:
//   OU exploration noise (noise.py:12-17) -> clip to +-0.999 (ddpg_train.py:151) -> power / phase map (:154-158) ->
//   get_next_phase (SENV:125-139) -> RIS cascade + step (SENV:149-171, 321-359) -> every agent's observation with its
//   theta slice (ddpg_train.py:47-73) -> remember (buffer.py:13-21).
// The staged path is sarl_action_map (torch), k_set_phase, the SARL step kernel, sarl_observe (torch): about ten launches,
// and theta written to HBM by one kernel to be read straight back by the next.
//
// Built on the latency-shaped family (k_step_lat.hip): the same FusedShape tiling, one memory round trip per wavefront,
// the same transposing butterfly -- so at the compile-time shapes the cascade sum comes out in the order of the SARL
// software pipeline (k_step_pipe.hip) and the outputs match the staged path bit for bit.  A wavefront owns EPWT envs:
//   1. requests, in the order of use: its lanes' step inputs, then mu / x / z of its envs' action rows (and, with the
//      ring, the observation rows it is about to replace), then b and EVERY h_r row of the first unit batch;
//   2. in the shadow of that round trip, two action elements per lane: noise, clip, map, exp(j phase) in float64 by the
//      routine k_set_phase uses.  x, action, phase and theta go to HBM (the env state stays coherent); theta, the powers
//      and the phase slices of the observation are parked in the wavefront's LDS slice;
//   3. the cascade reads theta from LDS -- never from HBM -- and sarl_core runs on the reduced sums, unchanged;
//   4. the observation rows are completed in LDS and leave as whole rows (obs_full, and the ring's new_state).
// LDS per workgroup, worst member (run-time M <= 256, four envs per wavefront): 32 KB theta + 19 KB observation rows.
#include "risvec_pipe.hpp"
#include "risvec_sarl.hpp"

namespace risvec {
namespace {

// OU update and clip of one element.  No contraction: tests restate these operations in NumPy float32, in this order.
__device__ __forceinline__ float ou_next(float x, float z, float th, float mu, float dt, float sig_sqdt) {
#pragma clang fp contract(off)
    const float drift = (th * (mu - x)) * dt;
    return (x + drift) + sig_sqdt * z;                                       // noise.py:13-14
}
__device__ __forceinline__ float clip_action(float s) {                      // ddpg_train.py:151 (NaN stays NaN, as np.clip)
    return s < -0.999f ? -0.999f : (s > 0.999f ? 0.999f : s);
}
__device__ __forceinline__ float unit_of(float a) {                          // ddpg_train.py:155-158: (a + 1) / 2
#pragma clang fp contract(off)
    return (a + 1.0f) * 0.5f;
}
__device__ __forceinline__ float phase_of(float a) {                         // ... * math.pi * 2 as float32, sarl_action_map's order
#pragma clang fp contract(off)
    return unit_of(a) * 6.2831855f;
}

// index of the env (0 .. EPWT-1) that word q of EPWT consecutive rows of `len` words belongs to
template <int EPWT>
__device__ __forceinline__ int row_of(int q, int len) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < EPWT; ++k) i += q >= k * len ? 1 : 0;
    return i;
}

template <class S, int EPWT, bool RING>
__global__ void __launch_bounds__(kBlock)
k_sarl_rollout(Dims d, RisVecSarlParams P, SarlArgs A, RisVecSarlRollout R, float* theta, long long head, uint32_t counter) {
    constexpr int V = S::V, VP = S::VP, G = S::G, NIT = S::NIT, VPP = S::VPP;
    constexpr int PC = S::PC, CHUNKS = S::CHUNKS, K = S::K;
    constexpr int NU = EPWT * CHUNKS;                          // load units of the wavefront's envs
    constexpr int NPMAX = S::FIXED ? S::MC / 2 : G * NIT;      // complex pairs per theta row this member can serve
    constexpr int PAMAX = V + NPMAX;                           // element pairs per action row
    constexpr int WMAX = 2 * NPMAX + 5 * V;                    // floats per obs_full row (V * (M / V) <= M)
    constexpr int NJ = (EPWT * PAMAX + kWave - 1) / kWave;     // action pairs per lane
    constexpr int NO = (EPWT * WMAX + kWave - 1) / kWave;      // observation words per lane
    constexpr int WPB = kBlock / kWave;
    static_assert(EPWT >= 1 && EPWT <= S::EPW, "a wavefront holds at most 64/VP envs");
    __shared__ __align__(16) float s_img[WPB][kWave * 2];
    __shared__ float4 s_theta[WPB][EPWT * NPMAX];              // theta rows of the wavefront's envs, two elements per entry
    __shared__ __align__(16) float s_pow[WPB][EPWT * 2 * V];                 // their power rows [p0 | p1]
    __shared__ float s_obs[WPB][EPWT * WMAX];                  // their obs_full rows

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gl = lane % G, gv = lane / G;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + wave);
    const int e0 = wid * EPWT;
    RISVEC_ARGS_IN_ONE_TRIP("s"(d.E), "s"(d.M), "s"(A.data_buf), "s"(A.pl), "s"(A.h_r), "s"(A.b), "s"(R.mu), "s"(R.ou_x),
                            "s"(R.z), "s"(R.obs_full));
    if (e0 >= d.E) return;                                     // a surplus wavefront of the last workgroup (whole wave)
    const int nenv = d.E - e0 < EPWT ? d.E - e0 : EPWT;        // wave-uniform
    const int M = S::FIXED ? S::MC : d.M;
    const int NP = M >> 1, PA = V + NP, tn = M / V, OW = tn + 5, W = V * OW;

    // (1) requests.  Every address is clamped into the wavefront's own rows: no branch around a load.
    const int i_mine = lane / VP, v_mine = lane % VP;
    const bool active = i_mine < nenv;
    const int e_mine = e0 + (active ? i_mine : 0);
    const long long idx = (long long)e_mine * V + v_mine;
    const float B = A.data_buf[idx], pl = A.pl[idx];

    const bool noise = R.ou_x != nullptr, injected = R.z != nullptr;
    const float2* __restrict__ mu2 = reinterpret_cast<const float2*>(R.mu) + (long long)e0 * PA;
    // (x / the observation rows are read here and rewritten below through other pointers: none of them is __restrict__)
    const float2* x2 = noise ? reinterpret_cast<const float2*>(R.ou_x) + (long long)e0 * PA : mu2;
    const float2* z2 = injected ? reinterpret_cast<const float2*>(R.z) + (long long)e0 * PA : mu2;
    const int npairs = nenv * PA, nobs = nenv * W;
    float2 mu[NJ], xo[NJ], zz[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
        const int q = lane + t * kWave, qc = q < npairs ? q : npairs - 1;
        mu[t] = mu2[qc];
        xo[t] = x2[qc];
        zz[t] = z2[qc];
    }
    float old[RING ? NO : 1];
    if constexpr (RING) {
        const float* of = R.obs_full + (long long)e0 * W;
#pragma unroll
        for (int t = 0; t < NO; ++t) {
            const int q = lane + t * kWave;
            old[t] = of[q < nobs ? q : nobs - 1];
        }
    }

    const float4* __restrict__ h4 = reinterpret_cast<const float4*>(A.h_r);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(A.b);
    float4 bq[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = gl + it * G;
        const float4 x = b4[p < NP ? p : NP - 1];
        bq[it] = p < NP ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ragged rows: lanes past the end re-read the row's last float4; their b is zero (k_step_pipe.hip)
    int pcl[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = gl + it * G;
        pcl[it] = (!S::RAGGED || p < NP) ? p : NP - 1;
    }
    const unsigned row_off = (unsigned)(gv * NP);
    const int e_last = d.E - 1;
    constexpr int UB = NU > 4 ? 4 : NU;
    static_assert(NU % UB == 0, "unit batches must tile the wavefront's units");
    float2 w0[NIT], w1[NIT];
#pragma unroll
    for (int b0 = 0; b0 < NU; b0 += UB) {
        float4 h[UB][PC][NIT];
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            const int ui = b0 + k;
            const int i = ui / CHUNKS, c = ui % CHUNKS;
            int e = e0 + i;
            e = e < e_last ? e : e_last;                       // tail: re-read the last env, masked later
            const float4* __restrict__ hb = h4 + (long long)e * (V * NP);
#pragma unroll
            for (int pc = 0; pc < PC; ++pc) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) h[k][pc][it] = hb[row_off + (unsigned)pcl[it] + ((c * PC + pc) * VPP * NP)];
            }
        }
        // (2) behind the last request of the first batch and in front of the first wait on h_r: the action rows
        if (b0 == 0) {
            const float sig_sqdt = R.ou_sigma * sqrtf(R.ou_dt);
            float2* xw = reinterpret_cast<float2*>(R.ou_x) + (long long)e0 * PA;
            float2* __restrict__ aw = reinterpret_cast<float2*>(R.action) + (long long)e0 * PA;
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                const int q = lane + t * kWave;
                const bool valid = q < npairs;
                const int i = row_of<EPWT>(q, PA), j = q - i * PA;            // env of the wavefront, pair of its row
                float2 a = mu[t];
                if (noise) {
                    float2 z = zz[t];
                    if (!injected) {
                        const uint4 r = philox4x32_10((uint32_t)(R.ou_env_offset + e0 + i), (uint32_t)j, counter, kSiteOU, R.ou_seed);
                        z = normal2(r.x, r.y);
                    }
                    const float2 xn = make_float2(ou_next(xo[t].x, z.x, R.ou_theta, R.ou_mu, R.ou_dt, sig_sqdt),
                                                  ou_next(xo[t].y, z.y, R.ou_theta, R.ou_mu, R.ou_dt, sig_sqdt));
                    if (valid) xw[q] = xn;
                    a = make_float2(a.x + xn.x, a.y + xn.y);                   // ddpg_torch.py:42
                }
                a = make_float2(clip_action(a.x), clip_action(a.y));
                if (!valid) continue;
                aw[q] = a;
                long long row = 0;
                if constexpr (RING) {
                    row = head + e0 + i;
                    row = row >= R.mem_size ? row - R.mem_size : row;
                    ring_st2(R.action_memory + row * (2 * PA) + 2 * j, a.x, a.y);
                }
                if (j < V) {                                                  // two powers: elements 2j, 2j + 1 of [p0 | p1]
                    *reinterpret_cast<float2*>(&s_pow[wave][i * 2 * V + 2 * j]) = make_float2(unit_of(a.x), unit_of(a.y));
                } else {                                                      // two phases: theta elements 2p, 2p + 1
                    const int p = j - V;
                    const float f0 = phase_of(a.x), f1 = phase_of(a.y);
                    const float2 t0 = phasor_of_angle(f0), t1 = phasor_of_angle(f1);
                    const float4 th = make_float4(t0.x, t0.y, t1.x, t1.y);
                    s_theta[wave][i * NP + p] = th;
                    const long long e = e0 + i;
                    reinterpret_cast<float4*>(theta)[e * NP + p] = th;      // state.theta stays coherent (SENV:125-131)
                    *reinterpret_cast<float2*>(R.phase + e * M + 2 * p) = make_float2(f0, f1);
                    // agent v's slice of the observation: phase[v tn : (v + 1) tn] (ddpg_train.py:50); the tail of the
                    // row beyond V tn belongs to nobody
                    const int m0 = 2 * p, va = m0 / tn, vb = (m0 + 1) / tn;
                    if (va < V) s_obs[wave][i * W + va * OW + (m0 - va * tn)] = f0;
                    if (vb < V) s_obs[wave][i * W + vb * OW + (m0 + 1 - vb * tn)] = f1;
                }
            }
            if constexpr (RING) {                                             // `state`: the rows as the kernel found them
#pragma unroll
                for (int t = 0; t < NO; ++t) {
                    const int q = lane + t * kWave;
                    if (q < nobs) {
                        const int i = row_of<EPWT>(q, W);
                        long long row = head + e0 + i;
                        row = row >= R.mem_size ? row - R.mem_size : row;
                        ring_st(R.state_memory + row * W + (q - i * W), old[t]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();                   // the wavefront's own LDS writes -> its reads (in order per wave)
        }
        // (3) the cascade, theta from LDS
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            const int ui = b0 + k;
            const int i = ui / CHUNKS, c = ui % CHUNKS;
            if (c == 0) {
                const int ic = i < nenv ? i : nenv - 1;        // rows of absent envs: any finite theta, masked later
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const float4 t = s_theta[wave][ic * NP + pcl[it]];
                    w0[it] = cmul(make_float2(t.x, t.y), make_float2(bq[it].x, bq[it].y));
                    w1[it] = cmul(make_float2(t.z, t.w), make_float2(bq[it].z, bq[it].w));
                }
            }
            float val[8];
#pragma unroll
            for (int pc = 0; pc < PC; ++pc) {
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    acc = cfma(make_float2(h[k][pc][it].x, h[k][pc][it].y), w0[it], acc);
                    acc = cfma(make_float2(h[k][pc][it].z, h[k][pc][it].w), w1[it], acc);
                }
                val[2 * pc] = acc.x;
                val[2 * pc + 1] = acc.y;
            }
            treduce<K, G / 2>(val, gl);
            if (gl % S::WSTRIDE == 0) {
                const int j = gl / S::WSTRIDE;
                const int v = (c * PC + (j >> 1)) * VPP + gv;
                s_img[wave][(i * VP + v) * 2 + (j & 1)] = val[0];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    const float2 img = *reinterpret_cast<const float2*>(&s_img[wave][lane * 2]);
    float g = 0.f, p0 = 0.f, p1 = 0.f;
    if (active) {
        g = gain_from_img(img, pl, nullptr, idx);
        A.gain[idx] = g;
        p0 = s_pow[wave][i_mine * 2 * V + v_mine];
        p1 = s_pow[wave][i_mine * 2 * V + V + v_mine];
    }
    const SarlOut o = sarl_core<VP>(d, P, A, e_mine, v_mine, active, g, p0, p1, active ? B : 0.f);

    // (4) the tail of this agent's observation (ddpg_train.py:54-71), then the rows leave whole
    if (active) {
        float* t5 = &s_obs[wave][i_mine * W + v_mine * OW + tn];
        t5[0] = o.data_buf * 0.1f; t5[1] = o.data_t * 0.1f; t5[2] = o.data_p * 0.1f; t5[3] = o.over_data * 0.1f;
        t5[4] = o.rate * 0.05f;
        if constexpr (RING) {
            if (v_mine == 0) {
                long long row = head + e_mine;
                row = row >= R.mem_size ? row - R.mem_size : row;
                ring_st(R.reward_memory + row, o.reward_mean);                // buffer.py:17
                R.terminal_memory[row] = (uint8_t)(R.done ? 1 : 0);
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    float* ow = R.obs_full + (long long)e0 * W;
#pragma unroll
    for (int t = 0; t < NO; ++t) {
        const int q = lane + t * kWave;
        if (q < nobs) {
            const float x = s_obs[wave][q];
            ow[q] = x;
            if constexpr (RING) {
                const int i = row_of<EPWT>(q, W);
                long long row = head + e0 + i;
                row = row >= R.mem_size ? row - R.mem_size : row;
                ring_st(R.new_state_memory + row * W + (q - i * W), x);
            }
        }
    }
}

template <class S, int EPWT>
hipError_t launch_member(const RisVecState& s, const RisVecSarlParams& p, const SarlArgs& a, const RisVecSarlRollout& r,
                         bool ring, uint32_t counter, hipStream_t st) {
    const long long waves = ((long long)s.n_envs + EPWT - 1) / EPWT;
    const unsigned grid = (unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave));
    const long long head = ring ? r.mem_cntr % r.mem_size : 0;
    if (S::FIXED) note_kernel("k_sarl_rollout<%d,%d,E%d%s>", S::V, S::MC, EPWT, ring ? ",RING" : "");
    else note_kernel("k_sarl_rollout<%d,G%d,N%d,E%d%s>", S::V, S::G, S::NIT, EPWT, ring ? ",RING" : "");
    if (ring) hipLaunchKernelGGL((k_sarl_rollout<S, EPWT, true>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), p, a, r, s.theta, head, counter);
    else hipLaunchKernelGGL((k_sarl_rollout<S, EPWT, false>), dim3(grid), dim3(kBlock), 0, st, dims_of(s), p, a, r, s.theta, head, counter);
    return hipGetLastError();
}

struct SarlSampleArgs {
    const float* state_memory; const float* action_memory; const float* reward_memory; const float* new_state_memory;
    const uint8_t* terminal_memory;
    long long max_mem;
    int batch, S, Ac;
    const int64_t* idx;
    uint64_t seed;
    uint32_t counter;
    float* states; float* actions; float* rewards; float* states_; uint8_t* dones;
    int64_t* idx_out;
};

// sample_buffer (buffer.py:23-34): one lane per output word; the row draw is risvec_replay_sample's
__global__ void __launch_bounds__(kBlock)
k_sarl_replay_sample(SarlSampleArgs A) {
    const long long S = A.S, Ac = A.Ac, n = A.batch;
    const long long b0 = n * S, b1 = b0 + n * Ac, b2 = b1 + n * S, b3 = b2 + n, b4 = b3 + n;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= b4) return;
    const auto row = [&](long long b) -> long long {
        if (A.idx) return A.idx[b];
        const uint32_t x = philox4x32_10((uint32_t)b, 0u, A.counter, kSiteReplay, A.seed).x;
        return (long long)(((unsigned long long)x * (unsigned long long)A.max_mem) >> 32);
    };
    if (gid < b0) {
        A.states[gid] = A.state_memory[row(gid / S) * S + gid % S];
    } else if (gid < b1) {
        const long long g = gid - b0;
        A.actions[g] = A.action_memory[row(g / Ac) * Ac + g % Ac];
    } else if (gid < b2) {
        const long long g = gid - b1;
        A.states_[g] = A.new_state_memory[row(g / S) * S + g % S];
    } else if (gid < b3) {
        const long long b = gid - b2, r = row(b);
        A.rewards[b] = A.reward_memory[r];
        if (A.idx_out) A.idx_out[b] = r;
    } else {
        const long long b = gid - b3;
        A.dones[b] = A.terminal_memory[row(b)];
    }
}

}  // namespace

// Shapes with a member: the latency-shaped family's (V in {4, 8, 16}, even M <= 256) with at least one phase per agent
bool sarl_rollout_covers(int V, int M) { return step_fused_lat_covers(V, M) && M >= V; }

hipError_t launch_sarl_rollout(const RisVecState& s, const RisVecSarlParams& p, const RisVecSarlRollout& r,
                               const int32_t* arrivals, uint64_t seed, uint32_t counter, hipStream_t st) {
    const int V = s.n_veh, M = s.n_ris;
    if (!sarl_rollout_covers(V, M)) return hipErrorNotSupported;
    SarlArgs a;
    a.action_power = nullptr; a.arrivals = arrivals; a.pl = s.pl; a.h_r = s.h_r; a.theta = s.theta;
    a.b = s.b; a.gain = s.gain; a.data_buf = s.data_buf; a.rate = s.rate; a.data_t = s.data_t;
    a.data_p = s.data_p; a.reward = s.reward; a.over_power = s.over_power; a.over_data = s.over_data;
    a.obs = s.obs; a.metrics = s.metrics; a.seed = seed; a.counter = counter; a.flags = RISVEC_STEP_OBS;
    const bool ring = r.state_memory != nullptr;
    // the compile-time members, each with the most envs per wavefront its latency-shaped kernel has, ...
#define RISVEC_X(VV, MM, DD, EMIN, EMAX, T) \
    if (V == VV && M == MM) return launch_member<FusedShape<VV, fused_g(VV, MM), fused_nit(VV, MM), MM>, EMAX>(s, p, a, r, ring, counter, st);
    RISVEC_FIXED_SHAPES(RISVEC_X)
#undef RISVEC_X
    // ... and the run-time-M member of every other even M
    const int g = fused_g(V, M), nit = fused_nit(V, M);
#define RISVEC_X(VV, GG, NN, EMIN, EMAX) \
    if (V == VV && g == GG && nit == NN) return launch_member<FusedShape<VV, GG, NN, 0>, EMAX>(s, p, a, r, ring, counter, st);
    RISVEC_RUNTIME_M_SHAPES(RISVEC_X)
#undef RISVEC_X
    return hipErrorNotSupported;
}

hipError_t launch_sarl_replay_sample(const RisVecSarlRollout& ring, int state_dims, int n_actions, long long max_mem,
                                     int batch, const int64_t* idx, uint64_t seed, uint32_t counter, float* states,
                                     float* actions, float* rewards, float* states_, uint8_t* dones, int64_t* idx_out,
                                     hipStream_t st) {
    const long long words = (long long)batch * (2LL * state_dims + n_actions + 2);
    const SarlSampleArgs a{ring.state_memory, ring.action_memory, ring.reward_memory, ring.new_state_memory,
                           ring.terminal_memory, max_mem, batch, state_dims, n_actions, idx, seed, counter,
                           states, actions, rewards, states_, dones, idx_out};
    hipLaunchKernelGGL(k_sarl_replay_sample, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace risvec
