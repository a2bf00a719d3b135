// K34, compile-time shapes: the fused "RIS cascaded gains + step()" kernel as a software
// pipeline.  Same results as the generic k_step_fused (k_step.hip), restructured so the
// HBM stream never waits for the step arithmetic:
//
//   * a wave owns SEVERAL groups of 64/VP envs (grid-strided), not one: while it runs
//     step() for group g, the h_r/theta loads of group g+1 are already in flight;
//   * loads are issued D "units" ahead (a unit = up to 4 vehicle rows of one env, i.e. up to
//     8 x 16-byte loads per lane) into a register ring that is indexed at compile time;
//   * the K = 2*PC per-lane partial sums of a unit (re/im of PC rows) are reduced with a
//     TRANSPOSING butterfly: at each of the first log2(K) steps a lane hands half of its
//     values to its partner and keeps the other half, so K values cost K-1 exchanges
//     instead of K*log2(G); exchanges at distance 1, 2, 4, 8 are DPP (plain VALU);
//   * step() inputs are fetched at the top of the group, long before they are needed.
//
// Reference: Simulation-MARL-BCD/Environment.py update_channel_gains ENV:263-273 + step
// ENV:547-731 (see risvec_step.hpp).
#include "risvec_pipe.hpp"
#include "risvec_sarl.hpp"

namespace risvec {

struct SarlIn {
    float p0, p1, B, pl;
};

struct SarlCore {
    static const char* name() { return "SarlCore"; }
    using Params = RisVecSarlParams;
    using Args = SarlArgs;
    using In = SarlIn;
    static __device__ __forceinline__ In load(const Dims& d, const Args& A, int e, int v, bool active) {
        In in{0.f, 0.f, 0.f, 0.f};
        if (active) {
            const long long idx = (long long)e * d.V + v;
            in.p0 = A.action_power[(long long)e * 2 * d.V + v];
            in.p1 = A.action_power[(long long)e * 2 * d.V + d.V + v];
            in.B = A.data_buf[idx];
            in.pl = A.pl[idx];
        }
        return in;
    }
    static __device__ __forceinline__ void hold(const In& in) {
        asm volatile("" ::"v"(in.p0), "v"(in.p1), "v"(in.B), "v"(in.pl));
    }
    template <int VP>
    static __device__ __forceinline__ void run(const Dims& d, const Params& P, const Args& A, int e, int v,
                                               bool active, float2 img, const In& in) {
        float g = 0.f;
        if (active) {
            const long long idx = (long long)e * d.V + v;
            g = gain_from_img(img, in.pl, nullptr, idx);
            A.gain[idx] = g;
        }
        sarl_core<VP>(d, P, A, e, v, active, g, in.p0, in.p1, in.B);
    }
};

struct GainArgs {
    const float* pl;
    const float* h_r;
    const float* theta;
    const float* b;
    const float* h_d;
    float* gain;
};

struct GainCore {
    static const char* name() { return "GainCore"; }
    using Params = int;
    using Args = GainArgs;
    struct In { float pl; };
    static __device__ __forceinline__ In load(const Dims& d, const Args& A, int e, int v, bool active) {
        return In{active ? A.pl[(long long)e * d.V + v] : 0.f};
    }
    static __device__ __forceinline__ void hold(const In& in) { asm volatile("" ::"v"(in.pl)); }
    template <int VP>
    static __device__ __forceinline__ void run(const Dims& d, const Params&, const Args& A, int e, int v,
                                               bool active, float2 img, const In& in) {
        if (active) {
            const long long idx = (long long)e * d.V + v;
            A.gain[idx] = gain_from_img(img, in.pl, A.h_d, idx);
        }
    }
};

// float4 load with the non-temporal hint (global_load ... nt): for a stream far larger than the 256 MiB Infinity
// Cache, allocating every line on its way through only evicts what somebody else could have reused
__device__ __forceinline__ float4 ld_nt(const float4* p) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}

// per_wave > 0: a wavefront owns the CONTIGUOUS groups [wid * per_wave, (wid + 1) * per_wave) -- it walks one
// contiguous piece of h_r from start to end; per_wave = 0: groups wid, wid + nw, ... (the round-1 form).
// NT: h_r / theta are read with the non-temporal hint.
//
// TK, theta by index (the cores whose Args are StepArgs): the env's phase shifts are read as candidate indices, one byte
// per element (A.theta_k = state.theta_idx: 2 bytes per lane and unit where the tensor costs 16), and expanded through
// the wavefront's 16-entry LDS table (theta_table_fill).  An instantiation of its own, chosen on the host (launch_pipe:
// A.theta_k != nullptr), like the latency family's TK and ALT: as a wave-uniform branch between two copies of the group
// loop inside one kernel the choice cost BOTH copies their registers (the kernel arguments ended up spilled to VGPR lanes:
// 87 SGPRs against 26, 697 v_readlane in the kernel against 48; EXPERIMENTS.md), and a test inside load_unit / do_group would
// be a join, which costs the counted s_waitcnt there (see the notes on ragged rows and on arrivals_src).  The form
// without TK never touches A.theta_k / A.theta_k_stride.
// NT + TK: the h_r rows keep the hint, the index loads use the default policy -- the index tensor is 64 B per env (16.8 MB
// at 262 144 envs), re-read every step, and fits the cache the hint is there to protect.
//
// REV, the backward walk (the cores whose Args are StepArgs, without NT): the wavefront owns the SAME groups and reads
// the same bytes, in the mirrored order -- its groups descending, the units of a group UPG-1 ... 0 (last env first, last
// chunk first), the row loads of a unit in descending address order.  The host alternates the two walks from step to
// step (launch_step: the step counter's parity), so what a wavefront read LAST in one launch is what it asks for FIRST in
// the next, while those lines are still close: a launch's tail is served faster to the next launch than the rest of the
// stream, and block -> XCD does not move between launches (tools/l2_carry_probe.py; EXPERIMENTS.md 2026-10-19, also on
// what the counters do and do not show about where the lines are found).  Which env a unit belongs to never enters
// the arithmetic, so the results are the forward walk's bit for bit.  An instantiation, not a flag: every ring slot,
// unit index and s_img address stays a compile-time constant, and there is no branch on the direction.
template <int V, int M, int D, class Core, bool NT = false, bool TK = false, bool REV = false>
__global__ void __launch_bounds__(kBlock)
k_step_fused_pipe(Dims d, typename Core::Params P, typename Core::Args A, int n_groups_total, int per_wave) {
    using In = typename Core::In;
    using S = PipeShape<V, M>;
    constexpr int VP = S::VP, EPW = S::EPW, NP = S::NP, G = S::G, NIT = S::NIT, VPP = S::VPP;
    constexpr int PC = S::PC, CHUNKS = S::CHUNKS, UPG = S::UPG, K = S::K;
    static_assert(!TK || std::is_same<typename Core::Args, StepArgs>::value, "theta by index: StepArgs carries the indices");
    static_assert(D <= UPG && UPG % D == 0, "ring depth must divide the units of a group");
    static_assert(!REV || (std::is_same<typename Core::Args, StepArgs>::value && !NT), "the backward walk: StepArgs cores, default policy");
    constexpr int C_FIRST = REV ? CHUNKS - 1 : 0;          // the chunk of an env that is served first: theta rides with it
    __shared__ float s_img[kBlock / kWave][kWave * 2];
    __shared__ float2 s_ph[TK ? kBlock / kWave : 1][16];       // TK: the 8 candidate phasors + the integer 0, per wavefront

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gl = lane % G, gv = lane / G;
    // wave-uniform by construction; tell the compiler so group indices live in SGPRs
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / kWave) + wave);
    const int nw = gridDim.x * (kBlock / kWave);
    const float4* __restrict__ h4 = reinterpret_cast<const float4*>(A.h_r);
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(A.theta);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(A.b);
    const int e_last = d.E - 1;
    float4 bq[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = gl + it * G;
        const float4 x = b4[p < NP ? p : NP - 1];
        bq[it] = p < NP ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // Ragged rows (NP % G != 0, i.e. M = 36 / 40: 18 / 20 float4 on 32 lanes): the lanes past the end of a row RE-READ
    // its last float4 instead of skipping the load.  A skipped load is a branch around the request with a zero fill
    // behind it, and the compiler can only order that fill against the loads in flight with `s_waitcnt vmcnt(0)` --
    // every unit then drains the whole ring (16 full drains per group in the M = 36 kernel, no counted wait left).
    // The re-read element shares its cache line with the row's last lane (no extra HBM traffic), and what those
    // lanes add to the sums is an exact +0: their b[m] is zero, so w0 / w1 are (signed) zeros, and +0 + (h * -0) = +0.
    int pcl[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = gl + it * G;
        pcl[it] = (NP % G == 0 || p < NP) ? p : NP - 1;
    }
    const unsigned row_off = (unsigned)(gv * NP);

    using U = Unit<PC, NIT, TK>;
    U ring[D];

    auto load_unit = [&](U& u, int grp, int ui) {
        const int i = ui / CHUNKS, c = ui % CHUNKS;
        int e = grp * EPW + i;
        e = e < e_last ? e : e_last;                       // tail: re-read the last env, masked later
        // wave-uniform 64-bit base (SGPRs) + 32-bit lane offset + compile-time constant:
        // the address arithmetic stays off the vector ALU
        const float4* __restrict__ hb = h4 + (long long)e * (V * NP);
        if constexpr (TK) {
            // the indices FIRST: loads return in issue order, so the table lookup can run while the unit's h_r rows
            // are still on their way
            if (c == C_FIRST) {
                const uint8_t* __restrict__ kb = A.theta_k + (long long)e * A.theta_k_stride;
#pragma unroll
                for (int k = 0; k < NIT; ++k) {
                    const int it = REV ? NIT - 1 - k : k;
                    u.k[it] = *reinterpret_cast<const uint16_t*>(kb + 2 * pcl[it]);
                }
            }
        }
        // (REV: the issue order is mirrored, every destination register is the one the forward walk uses)
#pragma unroll
        for (int kp = 0; kp < PC; ++kp) {
            const int pc = REV ? PC - 1 - kp : kp;
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int it = REV ? NIT - 1 - k : k;
                const float4* __restrict__ src = hb + (row_off + (unsigned)pcl[it] + ((c * PC + pc) * VPP * NP));
                u.h[pc][it] = NT ? ld_nt(src) : *src;
            }
        }
        if constexpr (!TK) {
            if (c == C_FIRST) {
                const float4* __restrict__ tb = t4 + (long long)e * NP;
#pragma unroll
                for (int k = 0; k < NIT; ++k) {
                    const int it = REV ? NIT - 1 - k : k;
                    u.t[it] = NT ? ld_nt(tb + pcl[it]) : tb[pcl[it]];
                }
            }
        }
    };

    // per_wave < 0 (experiment): the four wavefronts of a workgroup interleave over ONE contiguous range of
    // 4 * |per_wave| groups
    constexpr int WPB = kBlock / kWave;
    const int stride = per_wave > 0 ? 1 : (per_wave < 0 ? WPB : nw);
    int grp = per_wave > 0 ? wid * per_wave : (per_wave < 0 ? (wid / WPB) * (-per_wave * WPB) + (wid % WPB) : wid);
    int grp_end = per_wave > 0 ? grp + per_wave : (per_wave < 0 ? (wid / WPB + 1) * (-per_wave * WPB) : n_groups_total);
    grp_end = grp_end < n_groups_total ? grp_end : n_groups_total;
    // Fetch the kernel-argument pointers in the SAME scalar-load round trip as the exit condition: left alone, the
    // compiler loads n_groups_total first, waits, branches, and only then requests the pointers -- a second cold
    // scalar-cache miss (~0.35 us) in front of every wavefront's first HBM request.
    if constexpr (TK) {
        RISVEC_ARGS_IN_ONE_TRIP("s"(A.h_r), "s"(A.theta_k), "s"(A.theta_k_stride), "s"(A.b), "s"(n_groups_total), "s"(per_wave),
                                "s"(d.E));
    } else {
        RISVEC_ARGS_IN_ONE_TRIP("s"(A.h_r), "s"(A.theta), "s"(A.b), "s"(n_groups_total), "s"(per_wave), "s"(d.E));
    }
    if (grp >= grp_end) return;                            // whole wave: no cross-lane op is skipped
    // REV: start at the wavefront's last group and come down to its first.  A few scalar adds: a wavefront owns a handful
    // of groups (2 at the headline shape), and the count is not worth a division in front of the first request.
    const int grp_first = grp;
    if constexpr (REV) {
        while (grp + stride < grp_end) grp += stride;
    }
    // the unit served at position `pos` of a group's walk
    auto unit_at = [](int pos) { return REV ? UPG - 1 - pos : pos; };
#pragma unroll
    for (int pos = 0; pos < D; ++pos) load_unit(ring[pos], grp, unit_at(pos));
    if constexpr (TK) {
        theta_table_fill(s_ph[wave], lane);                // once per wavefront, behind the first requests
        __builtin_amdgcn_wave_barrier();                   // the wavefront's own table writes -> its reads
    }
    const int v_mine = lane % VP;

    // One group: consume its UPG units (refilling the ring D units ahead, across the group
    // boundary), prefetch the NEXT group's per-lane inputs into `in_nx`, then run the core with
    // `in`.  Called alternately with (inA, inB) / (inB, inA) so no register copy - and hence
    // no wait on the prefetch - is needed at the loop boundary.
    auto do_group = [&](int g_cur, const In& in, In& in_nx) {
        // The prefetch is unconditional (straight-line code keeps the compiler's vmcnt
        // bookkeeping exact): a wave on its last group "prefetches" group 0 instead, which
        // every such wave shares, so those requests are served by L2 and cost no HBM traffic.
        const int nxt = REV ? ((g_cur - stride >= grp_first) ? g_cur - stride : 0)
                            : ((g_cur + stride < grp_end) ? g_cur + stride : 0);
        const int e_mine = g_cur * EPW + lane / VP;
        const bool active = e_mine < d.E;
        // Take the wait for this group's per-lane inputs HERE (they were requested a whole
        // group ago), not at their first use inside the core, where the compiler could only
        // express it as vmcnt(0) and would drain the next group's prefetch with it.
        Core::hold(in);

        float2 w0[NIT], w1[NIT];
#pragma unroll
        for (int pos = 0; pos < UPG; ++pos) {
            U& u = ring[pos % D];
            const int ui = unit_at(pos);
            const int i = ui / CHUNKS, c = ui % CHUNKS;
            if (c == C_FIRST) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    float2 t0, t1;
                    if constexpr (TK) {
                        t0 = s_ph[wave][u.k[it] & 15u];
                        t1 = s_ph[wave][(u.k[it] >> 8) & 15u];
                    } else {
                        t0 = make_float2(u.t[it].x, u.t[it].y);
                        t1 = make_float2(u.t[it].z, u.t[it].w);
                    }
                    w0[it] = cmul(t0, make_float2(bq[it].x, bq[it].y));
                    w1[it] = cmul(t1, make_float2(bq[it].z, bq[it].w));
                }
            }
            float val[8];
            // (REV: the rows in the order they arrive; each row's sum is its own chain, so the bits do not move)
#pragma unroll
            for (int kp = 0; kp < PC; ++kp) {
                const int pc = REV ? PC - 1 - kp : kp;
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    acc = cfma(make_float2(u.h[pc][it].x, u.h[pc][it].y), w0[it], acc);
                    acc = cfma(make_float2(u.h[pc][it].z, u.h[pc][it].w), w1[it], acc);
                }
                val[2 * pc] = acc.x;
                val[2 * pc + 1] = acc.y;
            }
            treduce<K, G / 2>(val, gl);
            if (gl % S::WSTRIDE == 0) {
                const int j = gl / S::WSTRIDE;                 // value index = (row-in-unit, re/im)
                const int v = (c * PC + (j >> 1)) * VPP + gv;
                s_img[wave][(i * VP + v) * 2 + (j & 1)] = val[0];
            }
            // refill the slot just consumed, D units ahead (crossing into the next group)
            if (pos + D < UPG) load_unit(u, g_cur, unit_at(pos + D));
            else load_unit(u, nxt, unit_at(pos + D - UPG));
        }
        // per-lane inputs of the next group: in flight during this group's core
        in_nx = Core::load(d, A, nxt * EPW + lane / VP, v_mine, nxt * EPW + lane / VP < d.E);

        // the wave's own LDS writes -> its own reads (LDS is in-order per wave; no other wave
        // touches this slice); the barrier only pins the compiler's ordering
        __builtin_amdgcn_wave_barrier();
        const float2 img = *reinterpret_cast<const float2*>(&s_img[wave][lane * 2]);
        Core::template run<VP>(d, P, A, e_mine, v_mine, active, img, in);
        __builtin_amdgcn_wave_barrier();
    };

    In inA = Core::load(d, A, grp * EPW + lane / VP, v_mine, grp * EPW + lane / VP < d.E), inB;
    const int step = REV ? -stride : stride;
    auto done = [&](int g) { return REV ? g < grp_first : g >= grp_end; };
    while (true) {
        do_group(grp, inA, inB);
        grp += step;
        if (done(grp)) break;
        do_group(grp, inB, inA);
        grp += step;
        if (done(grp)) break;
    }
}

// Waves per CU to launch (each strides over groups) and ring depth.  Measured on MI355X at
// C3 (E=32768, V=8, M=64), ring depth D x waves/CU -> us per step:
//   D=1: 26.5 (8)  27.2 (12)  26.6 (16)      D=2: 27.0 (8)  26.7 (12)  26.3 (16)
//   D=4: 28.0 (4)  27.7 (8)   28.0 (12)      D=8: 29.7 (4)  29.7 (8)   29.6 (12)
// i.e. a shallow ring with more resident waves wins: deeper rings cost registers (fewer
// waves) and buy nothing once ~8 waves/CU already keep >= 16 KiB in flight each.
constexpr int kPipeWavesPerCu = 8;

// risvec_last_pipe_walk(): the walk of the calling thread's last pipeline launch (0 forward, 1 backward)
static thread_local int g_pipe_walk = 0;

// NT: non-temporal h_r / theta loads, once the per-step stream no longer fits the 256 MiB Infinity Cache (plan_pipe).
// Measured (same box, E x 8 x 64, us per step default / nt): 40 960 envs (188 MiB) 32.9 / 39.0, 57 344 (263 MiB)
// 46.0 / 53.8, 65 536 (288 MiB) 59.4 / 57.8, 262 144 (1.15 GiB) 245-250 / 221-223; 32 768 x 16 x 256 (1.1 GiB) with the
// BCD sweep 276-284 / 240-252 -- below the cache size the re-read of last step's lines is worth more than the hint,
// above it the hint is worth 10 %.
//
// rev: the backward walk (REV).  The direction is the caller's: launch_step alternates it from step to step.  Built for
// the cores that step on StepArgs, without NT; every other launch walks forward whatever `rev` says.
// RisVecForce::pipe_waves (tests): that many wavefronts instead, each with a CONTIGUOUS run of groups (per_wave > 0), so
// that one wavefront can own several groups at a few dozen envs.
template <int V, int M, int D, class Core>
static hipError_t launch_pipe(const RisVecState& s, const typename Core::Params& p, const typename Core::Args& a, bool nt,
                              bool rev, hipStream_t st) {
    using S = PipeShape<V, M>;
    const int n_groups = (s.n_envs + S::EPW - 1) / S::EPW;
    const int wpb = kBlock / kWave;
    const int forced_waves = forced_forms().pipe_waves;
    long long want_waves = forced_waves > 0 ? forced_waves : (long long)num_cus() * kPipeWavesPerCu;
    if (want_waves > n_groups) want_waves = n_groups;
    // balance: every wave gets the same number of groups (the last one possibly fewer)
    const long long per_wave = (n_groups + want_waves - 1) / want_waves;
    want_waves = (n_groups + per_wave - 1) / per_wave;
    const unsigned grid = (unsigned)((want_waves + wpb - 1) / wpb);
    const int contiguous = forced_waves > 0 ? (int)per_wave : 0;
    auto go = [&](auto knl) {
        hipLaunchKernelGGL(knl, dim3(grid), dim3(kBlock), 0, st, dims_of(s), p, a, n_groups, contiguous);
    };
    g_pipe_walk = 0;
    // the theta source and the walk are instantiations, picked here; the by-index and backward forms exist for the
    // cores that step on StepArgs
    if constexpr (std::is_same<typename Core::Args, StepArgs>::value) {
        if (rev && !nt) {
            if (a.theta_k != nullptr) go(k_step_fused_pipe<V, M, D, Core, false, true, true>);
            else go(k_step_fused_pipe<V, M, D, Core, false, false, true>);
            g_pipe_walk = 1;
            return hipGetLastError();
        }
        if (a.theta_k != nullptr) {
            if (nt) go(k_step_fused_pipe<V, M, D, Core, true, true>);
            else go(k_step_fused_pipe<V, M, D, Core, false, true>);
            return hipGetLastError();
        }
    }
    if (nt) go(k_step_fused_pipe<V, M, D, Core, true>);
    else go(k_step_fused_pipe<V, M, D, Core, false>);
    return hipGetLastError();
}

// Cores::at<V>: the core of that shape
template <class Core>
struct AnyV {
    template <int>
    using at = Core;
};
struct RingCores {
    template <int V>
    using at = MarlRingCore<V>;
};

// the compile-time shape of the plan (RISVEC_FIXED_SHAPES: one table for every core)
template <class Cores, class P, class A>
static hipError_t launch_pipe_shape(const RisVecState& s, const P& p, const A& a, const StepPlan& pl, bool rev,
                                    hipStream_t st) {
#define RISVEC_X(VV, MM, DD, EMIN, EMAX, T) \
    if (pl.V == VV && pl.M == MM) return launch_pipe<VV, MM, DD, typename Cores::template at<VV>>(s, p, a, pl.pol == 1, rev, st);
    RISVEC_FIXED_SHAPES(RISVEC_X)
#undef RISVEC_X
    return hipErrorNotSupported;
}

hipError_t launch_step_fused_pipe(const RisVecState& s, const RisVecParams& p, const StepArgs& a, const StepPlan& pl,
                                  bool rev, hipStream_t st) {
    if (pl.ring) return launch_pipe_shape<RingCores>(s, p, a, pl, rev, st);
    return launch_pipe_shape<AnyV<MarlCore>>(s, p, a, pl, rev, st);
}

int last_pipe_walk() { return g_pipe_walk; }
void note_pipe_walk(int walk) { g_pipe_walk = walk; }

template <class Core, class P, class A>
static hipError_t launch_core(const RisVecState& s, const P& p, const A& a, hipStream_t st) {
    const StepPlan pl = plan_pipe(s, Core::name());
    if (pl.family == StepPlan::NONE) return hipErrorNotSupported;
    const hipError_t err = launch_pipe_shape<AnyV<Core>>(s, p, a, pl, false, st);
    note_kernel("%s", pl.name);
    return err;
}

hipError_t launch_sarl_pipe(const RisVecState& s, const RisVecSarlParams& p, const SarlArgs& a, hipStream_t st) {
    return launch_core<SarlCore>(s, p, a, st);
}

hipError_t launch_gain_pipe(const RisVecState& s, hipStream_t st) {
    const GainArgs a{s.pl, s.h_r, s.theta, s.b, s.h_d, s.gain};
    return launch_core<GainCore>(s, 0, a, st);
}

}  // namespace risvec
