// K34-GEN, the software pipeline's member that REBUILDS the h_r rows instead of reading them
// (RISVEC_STEP_H_R_STEER_CURRENT).  compute_parms makes every row of h_r a pure function of one float64 angle per
// vehicle (k_geometry, k_env.hip); while that is still what state.h_r holds, the 8M bytes of a row need not be moved:
// steer_chunk() (risvec_dev.hpp) -- the routine k_geometry itself ran -- gives the same float32 elements from
// state.steer_ang (8 bytes) and state.z_r (16 bytes).  Everything behind the float4 is k_step_fused_pipe's, operation for
// operation: lane gl accumulates its NIT pairs with cfma from zero in `it` order, treduce<K, G/2>, the same s_img slot,
// the same core.  Only where the float4 comes from changes, so every output is the reading form's bit for bit.
//
// Two layouts share the file.  Where every wavefront owns ONE group and the shape keeps four wavefronts per SIMD
// (GenRowLane: 8 x 64 -- the headline --, 4 x 16, 16 x 64) a lane owns a whole ROW: gen_row_lane_form() below, whose
// comment has the layout and the order of its sums.  Everywhere else (more groups than wavefronts, 16 x 256) lanes own
// chunks and hand them over through LDS: gen_stage_form(), described here.
//
// The rotation chain inside a chunk is sequential (each step rounds), so a lane cannot start in the middle of one:
// lanes own WHOLE chunks.  One pass of the wavefront makes 64 chunks = 1024 consecutive elements of the group's rows
// (kWave / NCH rows, NCH = M / 16 chunks per row), parks each chunk's eight float4 in a per-wavefront LDS stage (chunk
// stride padded to 144 B against bank conflicts, as k_geometry's s_stage), and the consumer lanes read their float4 from
// the stage in the pipeline's layout (ds_read_b128 at compile-time offsets).  A group is NCH passes.  Same-wave LDS
// accesses execute in order, so __builtin_amdgcn_wave_barrier() between the stage's writes, its reads and the next
// pass's writes only pins the compiler; no workgroup barrier.
//
// What a pass needs from memory -- the angle and w of the lane's chunk, theta of the envs the pass completes -- is
// requested one outer iteration ahead (across the group boundary), step()'s per-lane inputs one group ahead as in the
// reading form.
//
// The kernel is bound by vector issue, not by bytes (EXPERIMENTS.md 2026-10-19 b), so what a wavefront issues beside the
// arithmetic of the result is kept out of it:
//   * step() reads some 25 pointers of StepArgs and 25 fields of RisVecParams.  Loaded at kernel entry they are live
//     across the pass loop, more than the scalar registers hold, and the compiler parked them in the lanes of a vector
//     register (v_writelane / v_readlane, a wait state each).  The passes need none of them, so step() reads them from
//     the kernel-argument segment AFTER the last pass (late_args below): the kernel takes its arguments as one struct so
//     that a field's place in the segment is its offsetof.
//   * ONE: the member for launches in which every wavefront owns one group (the headline: 4 096 groups on 4 096
//     wavefronts).  No group loop, no second set of step() inputs, no request for "the next group" -- and, in the
//     row-per-lane form, no stage, no s_img, no cross-lane reduce: what the stage layout costs beside the arithmetic
//     (16 + 16 ds_*_b128, the swaps, selects, DPP adds and their wait states per group) is not issued at all.
//   * HD (RISVEC_STEP_STEER_HEADS_CURRENT): the sincospi at the head of a chunk is a function of the angle alone, so
//     risvec_steer_heads() evaluates it once per geometry and the feed reads the float64 pair (steer_head() /
//     steer_chunk_from_head(), risvec_dev.hpp): 48 vector instructions per pass less, 16 bytes per lane and pass more.
//
// Every GEN member writes step()'s outputs non-temporal (GenStores).  The row-per-lane members draw the arrivals while
// their loads are in flight, and the headline among them runs a schedule of its own (GenRowSchedule).  Each of these was
// measured against its alternatives, which are no longer built: EXPERIMENTS.md has the figures and the commit they can
// be rebuilt from.  One build switch is left, the diagnostic RISVEC_GEN_STAMPS.
#include <cstddef>

#include "risvec_pipe.hpp"

// Diagnostic build only (Makefile: gen_stamps; tools/gen_wave_timeline.py): the row-per-lane members stamp s_memtime per
// wavefront into a buffer handed over through risvec_gen_stamps_buffer(), an entry point only that library has.  The
// shipped kernel executes no stamp.
#ifndef RISVEC_GEN_STAMPS
#define RISVEC_GEN_STAMPS 0
#endif

namespace risvec {

// How the GEN members write step()'s outputs (StorePolicy, risvec_step.hpp): every output with the non-temporal hint,
// row-lane and stage form, both cores.  A launch leaves 48 V + 68 bytes per env behind (14.8 MB at 32 768 x 8) and
// nothing on the device reads them before the launch ends; plain stores left them all dirty in L2 for the end of the
// launch to write back.  Measured against plain, write-through and write-through with the re-read tensors or obs left
// plain (EXPERIMENTS.md 2026-10-20 (d)).
using GenStores = StorePolicy<kStNonTemporal>;

// The priority of a row-lane wavefront that runs the priority schedule once `done` of its NL leaves (the blocks of
// row_tree that run chains) are behind it: min(3, NL) at entry, one level down per leaf, 0 from the third leaf on and
// through step().  Vector issue among the wavefronts of a SIMD goes by priority, then age, so with every wavefront at one
// level the oldest runs ahead and the youngest ends alone; keyed to progress, the one furthest behind is first in line.
constexpr int gen_prio_level(int NL, int done) {
    const int top = NL < 3 ? NL : 3;
    return done >= top ? 0 : top - done;
}

// The level to set once `done` leaves are behind, or -1 where the schedule has no change there.
constexpr int gen_prio_change(int NL, int done) {
    const int now = gen_prio_level(NL, done);
    return done == 0 || now != gen_prio_level(NL, done - 1) ? now : -1;
}

// row_tree_block() runs its leaves depth first, the far half of every fold behind the near one: leaf J is the
// bit-reversed-J-th of the G/8 blocks.  Its rank among the leaves that run chains (8 J < NP):
constexpr int gen_leaf_rank(int G, int NP, int J) {
    auto rev = [](int G_, int j) {
        int r = 0;
        for (int b = 1; b < G_ / 8; b <<= 1) r = (r << 1) | ((j & b) ? 1 : 0);
        return r;
    };
    int rank = 0;
    for (int j = 0; j < G / 8; ++j)
        if (8 * j < NP && rev(G, j) < rev(G, J)) ++rank;
    return rank;
}
constexpr int gen_leaf_count(int G, int NP) { return (NP < G ? NP : G) / 8; }

// Heads D leaves ahead.  Chunk c is read by leaf c % (G/8) (a leaf at NIT = 2 owns chunks J and J + G/8).  The rank at
// whose top -- behind the fence of the leaf before, in front of its first chain instruction -- the head of chunk c is
// requested, or -1: with the entry batch.  D = 0: every head at entry.  Otherwise the chunks of the first D leaves in
// execution order travel at entry and the others D leaves ahead of their own, so the entry burst of the launch (every
// wavefront of the grid within the same microsecond) carries D / NL of the heads' bytes.  The members use D = 0 and 1
// (GenRowSchedule); tests/test_gen_heads_ahead_host.py restates the rule for general D.
constexpr int gen_head_rank(int G, int NP, int D, int c) {
    const int own = gen_leaf_rank(G, NP, c % (G / 8));
    return D == 0 || own < D ? -1 : own - D;
}
// every chunk requested exactly once, at a rank below its own leaf's, and at entry exactly the first D leaves' chunks
constexpr bool gen_head_schedule_ok(int G, int NP, int D) {
    const int NL = gen_leaf_count(G, NP);
    for (int c = 0; c < NP / 8; ++c) {
        const int own = gen_leaf_rank(G, NP, c % (G / 8));
        int n = 0;
        for (int r = -1; r < NL; ++r)
            if (gen_head_rank(G, NP, D, c) == r) {
                ++n;
                if (r >= own) return false;
                if (D > 0 && (r == -1) != (own < D)) return false;
            }
        if (n != 1) return false;
    }
    return true;
}

// The stamps of a row-lane wavefront (RISVEC_GEN_STAMPS).  Per wavefront kGenStampSlots uint64: the stamps in order, then
// [12], [13] s_memrealtime at entry and end, [14] HW_REG_XCC_ID, [15] HW_REG_HW_ID | number of stamps << 32.
// mark_behind() first passes the registers a wait of interest is for through an empty asm, so that the wait stands in
// front of the stamp.  Without the switch every body is empty: no stamp, no pin.
constexpr int kGenStampMax = 12;
#if RISVEC_GEN_STAMPS
constexpr int kGenStampSlots = 16;
__device__ unsigned long long* g_gen_stamps = nullptr;
__device__ long long g_gen_stamps_waves = 0;
struct GenStamps {
    unsigned long long t[kGenStampMax];
    unsigned long long rt0;
    int n = 0;
    __device__ __forceinline__ void begin() {
        rt0 = __builtin_amdgcn_s_memrealtime();
        mark();
    }
    __device__ __forceinline__ void mark() { t[n++] = __builtin_amdgcn_s_memtime(); }
    template <class T0, class T1>
    __device__ __forceinline__ void mark_behind(T0& v0, T1& v1) {
        asm volatile("" : "+v"(v0), "+v"(v1));
        mark();
    }
    __device__ __forceinline__ void mark_behind_scalar(int s) {
        asm volatile("" : "+s"(s));
        mark();
    }
    // behind the wavefront's last store: the closing stamp, and lane 0 writes the wavefront's slots (n_all stamps)
    __device__ __forceinline__ void finish(int wid, int lane, int n_all) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        mark();
        const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long* __restrict__ out = g_gen_stamps;
        if (out != nullptr && wid < g_gen_stamps_waves && lane == 0) {
            out += (long long)wid * kGenStampSlots;
#pragma unroll
            for (int i = 0; i < n_all; ++i) out[i] = t[i];
            out[12] = rt0;
            out[13] = rt1;
            out[14] = __builtin_amdgcn_s_getreg(20 | (31 << 11));                                  // HW_REG_XCC_ID
            out[15] = (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11))      // HW_REG_HW_ID
                      | ((unsigned long long)n_all << 32);
        }
    }
};
#else
struct GenStamps {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void mark() {}
    template <class T0, class T1>
    __device__ __forceinline__ void mark_behind(T0&, T1&) {}
    __device__ __forceinline__ void mark_behind_scalar(int) {}
    __device__ __forceinline__ void finish(int, int, int) {}
};
#endif

template <int V, int M>
struct GenShape : PipeShape<V, M> {
    using S = PipeShape<V, M>;
    static_assert(M % kGeoChunk == 0, "rows are rebuilt in whole 16-element chunks");
    static_assert(S::EPW * V == kWave, "a group is 64 rows");
    static constexpr int NCH = M / kGeoChunk;                  // chunks per row = passes per group
    static_assert(NCH <= kWave, "a pass must cover at least one row");
    static constexpr int RPP = kWave / NCH;                    // rows per pass
    static constexpr int RPU = S::PC * S::VPP;                 // rows per unit (units partition the group's rows in order)
    static_assert(RPP % RPU == 0, "a pass must hold whole units");
    static constexpr int UPP = RPP / RPU;                      // units per pass
    // an outer iteration = SP passes = whole envs, so which chunk of an env a unit is stays a compile-time constant
    static constexpr int SP = UPP >= S::CHUNKS ? 1 : S::CHUNKS / UPP;
    static constexpr int EPO = SP * UPP / S::CHUNKS;           // envs per outer iteration
    static constexpr int NO = NCH / SP;                        // outer iterations per group
    static_assert(SP * UPP % S::CHUNKS == 0 && NCH % SP == 0 && NO * EPO == S::EPW, "outer iterations must tile the group");
    static constexpr int STAGE = kWave * (kGeoChunk / 2 + 1);  // float4 per wavefront: 64 chunks of 8 (+1 pad)
};

// The headline member: the plain MARL core at 8 x 64 (bench.py's default workload).  It alone takes the schedule below,
// because that is where each part of it was measured to pay (EXPERIMENTS.md 2026-10-21 (c), (d)).  The ring core
// (bench.py --replay: a long tail of stores behind the chains) LOSES with each part -- 11 % with the priority levels,
// whose stagger is what puts one wavefront's stores under the others' chains, 5 ... 7 % with the heads a leaf ahead, with
// or without the late inputs -- and 4 x 16 and 16 x 64 run as one-group launches in no benchmark leg: unmeasured.
template <int V, int M, class Core>
constexpr bool gen_headline_member() {
    return std::is_same<Core, MarlCore>::value && V == 8 && M == 64;
}

// When a row-lane member (gen_row_lane_form) asks for what and at which priority its wavefronts run.  Every other member
// than the headline sets no priority and requests everything a lane reads in one batch at entry.
template <int V, int M, class Core, bool HD>
struct GenRowSchedule {
    using S = GenShape<V, M>;
    static constexpr int NL = gen_leaf_count(S::G, S::NP);     // leaves that run chains
    // wave priority by progress (gen_prio_level), each level the text of a statement that stands there anyway
    static constexpr bool prio = gen_headline_member<V, M, Core>();
    // only HD members have heads: the head of a chunk requested heads_ahead leaves ahead of the leaf that starts from it
    // (gen_head_rank), 0: all NCH at entry
    static constexpr int heads_ahead = HD && gen_headline_member<V, M, Core>() ? 1 : 0;
    // step()'s inputs requested at the top of the leaf of rank in_rank and held at the top of the leaf after it, not at entry
    static constexpr bool late_in = HD && gen_headline_member<V, M, Core>();
    static constexpr int in_rank = NL < 2 ? NL - 1 : 1;
    // the level to set once `done` leaves are behind, or -1: none
    static constexpr int prio_change(int done) { return prio ? gen_prio_change(NL, done) : -1; }
    static_assert(gen_head_schedule_ok(S::G, S::NP, 0) && gen_head_schedule_ok(S::G, S::NP, 1),
                  "every chunk's head is requested once, below its own leaf's rank");
};

// what one outer iteration reads from memory: per pass the lane's chunk -- its row's angle, or (HD) the chunk's head as
// risvec_steer_heads stored it -- and the row's w; per env theta or its indices
template <int SP, bool HD>
struct GenRows {
    double ang[SP];
    double2 w[SP];
};
template <int SP>
struct GenRows<SP, true> {
    double2 head[SP];
    double2 w[SP];
};
template <int SP, int EPO, int NIT, bool TK, bool HD>
struct GenFeed : GenRows<SP, HD> {
    float4 t[EPO][NIT];
};
template <int SP, int EPO, int NIT, bool HD>
struct GenFeed<SP, EPO, NIT, true, HD> : GenRows<SP, HD> {
    unsigned k[EPO][NIT];
};

// The kernel's ONLY parameter, so that the kernel-argument segment is this struct and a field sits at its offsetof.
// per_wave > 0: a wavefront owns the CONTIGUOUS groups [wid * per_wave, (wid + 1) * per_wave); per_wave = 0: groups
// wid, wid + nw, ...
// rev: the wavefront serves the SAME groups, last first -- the pipeline's alternating walk (launch_step: the parity of the
// step counter), kept so that what a launch touched last (theta or its indices, step()'s inputs: all that is still read)
// is what the next launch asks for first.  Only the order of the groups turns: nothing inside a group depends on the
// direction, so it is a run-time argument here, not an instantiation.
template <class Core>
struct GenArgs {
    Dims d;
    typename Core::Params P;
    typename Core::Args A;
    const double* steer;            // HD: the chunk heads [E,V,M/16] complex128, else state.steer_ang [E,V]
    const double* z_r;
    int n_groups_total, per_wave, rev;
};

// The kernel's arguments again, as the segment holds them: the address is taken anew and passed through an empty asm, so
// the compiler cannot tell these loads from others and issues them HERE (scalar loads: the constant address space
// survives the cast), not at kernel entry next to the ones the prologue makes from the parameter itself.
template <class Core>
__device__ __forceinline__ const GenArgs<Core>& late_args() {
    static_assert(offsetof(GenArgs<Core>, d) == 0 && std::is_trivially_copyable<GenArgs<Core>>::value,
                  "the kernel-argument segment must be the struct itself");
    typedef const __attribute__((address_space(4))) GenArgs<Core>* SegPtr;
    SegPtr seg = (SegPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(seg));
    return *(const GenArgs<Core>*)seg;
}

// The arguments of a member's first requests in one scalar round trip (RISVEC_ARGS_IN_ONE_TRIP), in the names both forms
// give them (steer, KA, A, n_groups_total, d; TK picks theta's source).  A statement, not a function: `text` is what the
// row-lane form's entry priority level is written into (RISVEC_GEN_FENCE has the reason), and further operands follow a
// comma: RISVEC_GEN_FIRST_ARGS("", ) or RISVEC_GEN_FIRST_ARGS("...", , operand, ...).
#define RISVEC_GEN_FIRST_ARGS(text, ...)                                                                                   \
    if constexpr (TK) {                                                                                                    \
        asm volatile(text ::"s"(steer), "s"(KA.z_r), "s"(A.theta_k), "s"(A.theta_k_stride), "s"(A.b), "s"(n_groups_total), \
                     "s"(d.E)__VA_ARGS__);                                                                                 \
    } else {                                                                                                               \
        asm volatile(text ::"s"(steer), "s"(KA.z_r), "s"(A.theta), "s"(A.b), "s"(n_groups_total), "s"(d.E)__VA_ARGS__);    \
    }

// The fence behind a chain of the row-lane form's leaf: its eight partials `acc` pass through an asm that clobbers memory.
// A change of wave priority is the TEXT of the leaf's last fence, not an instruction of its own: the compiler sees the
// same statement with the same operands wherever the text is empty or not, so nothing else moves.
// (__builtin_amdgcn_s_setprio ends a scheduling region: with it the M = 64 members need 115 ... 146 registers instead of
// 93 ... 122 and the ring core loses its fourth wavefront.)  Hence a macro: the text of an asm must be a literal.
#define RISVEC_GEN_FENCE(acc, text, ...)                                                                                   \
    asm volatile(text : "+v"(acc[0].x), "+v"(acc[0].y), "+v"(acc[1].x), "+v"(acc[1].y), "+v"(acc[2].x), "+v"(acc[2].y),    \
                        "+v"(acc[3].x), "+v"(acc[3].y), "+v"(acc[4].x), "+v"(acc[4].y), "+v"(acc[5].x), "+v"(acc[5].y),    \
                        "+v"(acc[6].x), "+v"(acc[6].y), "+v"(acc[7].x), "+v"(acc[7].y)                                     \
                 : __VA_ARGS__                                                                                             \
                 : "memory")

// TK: theta by index, as in k_step_fused_pipe.  ONE: every wavefront owns one group (group `wid`; per_wave and rev are
// not read).  HD (RISVEC_STEP_STEER_HEADS_CURRENT): the head of a chunk, exp(-j pi ang m0) in float64, is a function of
// the angle alone and changes only when the geometry does, so it is read (16 B per lane and pass, the heads of a pass
// contiguous) instead of evaluated by sincospi 64 lanes x NCH passes x every launch; the rotations start from the same
// float64 pair either way.  steer_ang is not read then.
template <int V, int M, class Core, bool TK, bool ONE, bool HD>
__device__ __forceinline__ void gen_stage_form(const GenArgs<Core>& KA) {
    using In = typename Core::In;
    using S = GenShape<V, M>;
    constexpr int VP = S::VP, EPW = S::EPW, NP = S::NP, G = S::G, NIT = S::NIT, VPP = S::VPP;
    constexpr int PC = S::PC, CHUNKS = S::CHUNKS, K = S::K;
    constexpr int NCH = S::NCH, RPP = S::RPP, RPU = S::RPU, UPP = S::UPP, SP = S::SP, EPO = S::EPO, NO = S::NO;
    static_assert(std::is_same<typename Core::Args, StepArgs>::value, "the GEN members step on StepArgs");
    using Feed = GenFeed<SP, EPO, NIT, TK, HD>;
    __shared__ float s_img[kBlock / kWave][kWave * 2];
    __shared__ float2 s_ph[TK ? kBlock / kWave : 1][16];
    __shared__ float4 s_stage[kBlock / kWave][S::STAGE];

    // the prologue's view of the arguments: what is named here is loaded at entry.  step() goes through late_args().
    const Dims& d = KA.d;
    const typename Core::Args& A = KA.A;
    const double* __restrict__ steer = KA.steer;
    const int n_groups_total = KA.n_groups_total;

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int gl = lane % G, gv = lane / G;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / kWave) + wave);
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(A.theta);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(A.b);
    const double2* __restrict__ z2 = reinterpret_cast<const double2*>(KA.z_r);
    const int e_last = d.E - 1;
    const int row_last = d.E * V - 1;
    float4 bq[NIT];
    int pcl[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int p = gl + it * G;
        const float4 x = b4[p < NP ? p : NP - 1];
        bq[it] = p < NP ? x : make_float4(0.f, 0.f, 0.f, 0.f);
        // (ragged rows, NP % G != 0: the lanes past the end of a row take its last float4, against a zero b -- an exact
        // +0 in the sums, as in the reading form)
        pcl[it] = (NP % G == 0 || p < NP) ? p : NP - 1;
    }
    // producer: this lane's chunk of a pass -- row lane / NCH of the pass, elements m0 ...
    const int p_row = lane / NCH, p_ch = lane % NCH, p_m0 = p_ch * kGeoChunk;
    float4* __restrict__ stage = s_stage[wave];
    float4* __restrict__ p_dst = stage + lane * (kGeoChunk / 2 + 1);
    // consumer: float4 `pcl[it]` of row gv of a unit's lane-group pass, as an index into the stage (8 float4 per chunk,
    // chunk stride 9); the unit and the row-in-unit add compile-time offsets
    const float4* c_src[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int f = gv * NP + pcl[it];
        c_src[it] = stage + (f >> 3) * (kGeoChunk / 2 + 1) + (f & 7);
    }

    // the requests of outer iteration `o` of group `grp` (tail: the last row / env again, masked later)
    auto load_feed = [&](Feed& f, int grp, int o) {
#pragma unroll
        for (int sp = 0; sp < SP; ++sp) {
            int row = grp * kWave + (o * SP + sp) * RPP + p_row;
            row = row < row_last ? row : row_last;
            if constexpr (HD) f.head[sp] = reinterpret_cast<const double2*>(steer)[(long long)row * NCH + p_ch];
            else f.ang[sp] = steer[row];
            f.w[sp] = z2[row];
        }
#pragma unroll
        for (int ie = 0; ie < EPO; ++ie) {
            int e = grp * EPW + o * EPO + ie;
            e = e < e_last ? e : e_last;
            if constexpr (TK) {
                const uint8_t* __restrict__ kb = A.theta_k + (long long)e * A.theta_k_stride;
#pragma unroll
                for (int it = 0; it < NIT; ++it) f.k[ie][it] = *reinterpret_cast<const uint16_t*>(kb + 2 * pcl[it]);
            } else {
                const float4* __restrict__ tb = t4 + (long long)e * NP;
#pragma unroll
                for (int it = 0; it < NIT; ++it) f.t[ie][it] = tb[pcl[it]];
            }
        }
    };

    // outer iteration `o` of a group on the feed `cur`: SP passes, each a stage of 64 chunks made and consumed
    auto do_outer = [&](int o, const Feed& cur) {
        float2 w0[NIT], w1[NIT];
#pragma unroll
        for (int sp = 0; sp < SP; ++sp) {
            float4 q[kGeoChunk / 2];
            if constexpr (HD) steer_chunk_from_head(cur.head[sp].x, cur.head[sp].y, cur.w[sp].x, cur.w[sp].y, q);
            else steer_chunk(cur.ang[sp], cur.w[sp].x, cur.w[sp].y, p_m0, q);
#pragma unroll
            for (int k = 0; k < kGeoChunk / 2; ++k) p_dst[k] = q[k];
            __builtin_amdgcn_wave_barrier();           // the stage's writes -> its reads (same wave: in order)
#pragma unroll
            for (int ul = 0; ul < UPP; ++ul) {
                const int uo = sp * UPP + ul;          // unit within the outer iteration
                const int c = uo % CHUNKS, ie = uo / CHUNKS;
                if (c == 0) {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        float2 t0, t1;
                        if constexpr (TK) {
                            t0 = s_ph[wave][cur.k[ie][it] & 15u];
                            t1 = s_ph[wave][(cur.k[ie][it] >> 8) & 15u];
                        } else {
                            t0 = make_float2(cur.t[ie][it].x, cur.t[ie][it].y);
                            t1 = make_float2(cur.t[ie][it].z, cur.t[ie][it].w);
                        }
                        w0[it] = cmul(t0, make_float2(bq[it].x, bq[it].y));
                        w1[it] = cmul(t1, make_float2(bq[it].z, bq[it].w));
                    }
                }
                float val[8];
#pragma unroll
                for (int pc = 0; pc < PC; ++pc) {
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const float4 h = c_src[it][((ul * RPU + pc * VPP) * NCH) * (kGeoChunk / 2 + 1)];
                        acc = cfma(make_float2(h.x, h.y), w0[it], acc);
                        acc = cfma(make_float2(h.z, h.w), w1[it], acc);
                    }
                    val[2 * pc] = acc.x;
                    val[2 * pc + 1] = acc.y;
                }
                treduce<K, G / 2>(val, gl);
                if (gl % S::WSTRIDE == 0) {
                    const int j = gl / S::WSTRIDE;             // value index = (row-in-unit, re/im)
                    const int v = (c * PC + (j >> 1)) * VPP + gv;
                    const int i = o * EPO + ie;                // env of the group
                    s_img[wave][(i * VP + v) * 2 + (j & 1)] = val[0];
                }
            }
            __builtin_amdgcn_wave_barrier();           // the stage's reads -> the next pass's writes
        }
    };

    const int v_mine = lane % VP;

    if constexpr (ONE) {
        RISVEC_GEN_FIRST_ARGS("", )
        const int grp = wid;
        if (grp >= n_groups_total) return;                     // whole wave: no cross-lane op is skipped
        Feed cur;
        load_feed(cur, grp, 0);
        if constexpr (TK) {
            theta_table_fill(s_ph[wave], lane);
            __builtin_amdgcn_wave_barrier();
        }
        const int e_mine = grp * EPW + lane / VP;
        const bool active = e_mine < d.E;
        const In in = Core::load(d, A, e_mine, v_mine, active);
        Core::hold(in);
        // the last outer iteration is peeled: nothing is requested behind it
#pragma unroll 1
        for (int o = 0; o + 1 < NO; ++o) {
            Feed nx;
            load_feed(nx, grp, o + 1);
            do_outer(o, cur);
            cur = nx;
        }
        do_outer(NO - 1, cur);

        const GenArgs<Core>& L = late_args<Core>();
        __builtin_amdgcn_wave_barrier();
        const float2 img = *reinterpret_cast<const float2*>(&s_img[wave][lane * 2]);
        Core::template run<VP, GenStores>(L.d, L.P, L.A, e_mine, v_mine, active, img, in);
    } else {
        const int per_wave = KA.per_wave;
        const int nw = gridDim.x * (kBlock / kWave);
        const int stride = per_wave > 0 ? 1 : nw;
        int grp = per_wave > 0 ? wid * per_wave : wid;
        int grp_end = per_wave > 0 ? grp + per_wave : n_groups_total;
        grp_end = grp_end < n_groups_total ? grp_end : n_groups_total;
        RISVEC_GEN_FIRST_ARGS("", , "s"(per_wave))
        if (grp >= grp_end) return;                            // whole wave: no cross-lane op is skipped
        const int grp_first = grp;
        if (KA.rev) {                                          // a few scalar adds: a wavefront owns a handful of groups
            while (grp + stride < grp_end) grp += stride;
        }
        const int step = KA.rev ? -stride : stride;
        Feed cur;
        load_feed(cur, grp, 0);
        if constexpr (TK) {
            theta_table_fill(s_ph[wave], lane);
            __builtin_amdgcn_wave_barrier();
        }

        auto do_group = [&](int g_cur, const In& in, In& in_nx) {
            // (unconditional prefetches, as in the reading form: a wave on its last group asks for group 0's)
            const int g_nx = g_cur + step;
            const int nxt = (g_nx >= grp_first && g_nx < grp_end) ? g_nx : 0;
            const int e_mine = g_cur * EPW + lane / VP;
            const bool active = e_mine < d.E;
            Core::hold(in);

#pragma unroll 1
            for (int o = 0; o < NO; ++o) {
                Feed nx;
                if (o + 1 < NO) load_feed(nx, g_cur, o + 1);
                else load_feed(nx, nxt, 0);
                do_outer(o, cur);
                cur = nx;
            }
            const GenArgs<Core>& L = late_args<Core>();
            in_nx = Core::load(L.d, L.A, nxt * EPW + lane / VP, v_mine, nxt * EPW + lane / VP < L.d.E);

            __builtin_amdgcn_wave_barrier();
            const float2 img = *reinterpret_cast<const float2*>(&s_img[wave][lane * 2]);
            Core::template run<VP, GenStores>(L.d, L.P, L.A, e_mine, v_mine, active, img, in);
            __builtin_amdgcn_wave_barrier();
        };

        In inA = Core::load(d, A, grp * EPW + lane / VP, v_mine, grp * EPW + lane / VP < d.E), inB;
        while (true) {
            do_group(grp, inA, inB);
            grp += step;
            if (grp < grp_first || grp >= grp_end) break;
            do_group(grp, inB, inA);
            grp += step;
            if (grp < grp_first || grp >= grp_end) break;
        }
    }
}

// ---------------------------------------------------------------------------
// The row-per-lane form of the one-group member.  A group is 64 rows and step() runs with lane = (env lane / V, vehicle
// lane % V), which IS the row index: the lane that rebuilds a row also consumes it.  It runs the row's NCH chunk chains
// (the same float64 work per wavefront as a pass per chunk), multiplies each float4 by the env's w = theta * b as it
// leaves the chain, and adds the partials in registers in the order the reading form's treduce<K, G/2> adds them across
// lanes -- so the reduced img is already in the lane that runs step(), with no stage, no s_img, no cross-lane exchange.
//
// The tree.  In the reading form lane gl of a row chains its NIT float4 from zero (cfma, `it` order) into the partial
// p[gl]; treduce then adds pairwise at distance O = G/2, ..., 1 with xchg<O>'s partners: gl ^ O, except the DPP mirrors at
// O = 8 (g <-> 15 - g within 16) and O = 4 (g <-> 7 - g within 8).  Which lane keeps and which sends does not matter (a
// float add commutes), so with s_G = p the sums are
//     s_O[g] = s_2O[g] + s_2O[O == 8 || O == 4 ? 2 O - 1 - g : g + O],   g < O,
// and s_1[0] is what the writer lane held.  row_tree_block() evaluates s_O in blocks of 8 consecutive g -- a leaf block is
// one chunk (and the chunk G/8 behind it where NIT = 2) -- depth first, so that partners at the largest distance fold
// first and few blocks are live.  Ragged rows (NP < G): the reading form's lanes past the end of a row form their
// partial against b = 0, an exact +0 (fma(h, +-0, +0) is +0 for every finite h); those blocks are +0 here too and are
// added, not skipped.
// ---------------------------------------------------------------------------
template <int G, int O, int J, class Leaf>
__device__ __forceinline__ void row_tree_block(float2 (&out)[8], Leaf&& leaf) {
    if constexpr (O == G) {
        leaf(std::integral_constant<int, J>{}, out);
    } else if constexpr (O >= 16) {
        float2 far[8];
        row_tree_block<G, 2 * O, J>(out, leaf);
        row_tree_block<G, 2 * O, J + O / 8>(far, leaf);
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = make_float2(out[k].x + far[k].x, out[k].y + far[k].y);
    } else {
        static_assert(O == 8 && J == 0, "below 16 the values of a row sit in one block");
        float2 far[8];
        row_tree_block<G, 16, 0>(out, leaf);
        row_tree_block<G, 16, 1>(far, leaf);
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = make_float2(out[k].x + far[7 - k].x, out[k].y + far[7 - k].y);
    }
}

template <int G, class Leaf>
__device__ __forceinline__ float2 row_tree(Leaf&& leaf) {
    static_assert(G == 16 || G == 32 || G == 64, "treduce<K, G/2> starts at distance 8, 16 or 32");
    float2 s[8];
    row_tree_block<G, 8, 0>(s, leaf);
#pragma unroll
    for (int g = 0; g < 4; ++g) s[g] = make_float2(s[g].x + s[7 - g].x, s[g].y + s[7 - g].y);       // O = 4: the half mirror
#pragma unroll
    for (int g = 0; g < 2; ++g) s[g] = make_float2(s[g].x + s[g + 2].x, s[g].y + s[g + 2].y);       // O = 2
    return make_float2(s[0].x + s[1].x, s[0].y + s[1].y);                                           // O = 1
}

// the theta indices of Q float4 (2 Q bytes, Q even), as one aligned load: theta_idx_stride() is a multiple of 32
template <int Q>
struct alignas(2 * Q) GenIdx {
    unsigned w[Q / 2];
};

template <int V, int M, class Core, bool TK, bool HD>
__device__ __forceinline__ void gen_row_lane_form(const GenArgs<Core>& KA) {
    using In = typename Core::In;
    using S = GenShape<V, M>;
    constexpr int VP = S::VP, EPW = S::EPW, NP = S::NP, G = S::G, NIT = S::NIT, NCH = S::NCH;
    static_assert(std::is_same<typename Core::Args, StepArgs>::value, "the GEN members step on StepArgs");
    static_assert(VP == V && EPW * V == kWave, "lane = row of the group");
    static_assert(NP % V == 0 && (NP / V) % 2 == 0, "an env's w is made by its V lanes, an even share each");
    static_assert(NP % G == 0 || NIT == 1, "ragged rows: whole blocks past the end of the row");
    constexpr int Q = NP / V;                                  // float4 of w per lane
    constexpr int WS = NP + 1;                                 // env stride of s_w: the EPW addresses of a read on their own banks
    __shared__ float4 s_w[kBlock / kWave][EPW * WS];
    __shared__ float2 s_ph[TK ? kBlock / kWave : 1][16];

    const Dims& d = KA.d;
    const typename Core::Args& A = KA.A;
    const double* __restrict__ steer = KA.steer;
    const int n_groups_total = KA.n_groups_total;

    using SCH = GenRowSchedule<V, M, Core, HD>;
    constexpr int NL = SCH::NL;                                // leaves that run chains
    constexpr int D = SCH::heads_ahead;                        // heads requested D leaves ahead (0: all at entry)
    constexpr bool LATE = SCH::late_in;                        // step()'s inputs at the top of the leaf of rank IN_RANK
    constexpr int IN_RANK = SCH::in_rank;
    GenStamps ts;
    ts.begin();                                                // entry

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / kWave) + wave);
    // The entry level of the priority schedule is the text of the argument batch, in front of the first request to memory.
    constexpr int level0 = SCH::prio_change(0);
    if constexpr (level0 >= 0) {
        RISVEC_GEN_FIRST_ARGS("s_setprio %[level]", , [level] "n"(level0))
    } else {
        RISVEC_GEN_FIRST_ARGS("", )
    }
    const int grp = wid;
    if (grp >= n_groups_total) return;                         // whole wave

    // everything the lane reads, in one batch (tail: the last row / env again, masked by `active`)
    const int v_mine = lane % VP, i_env = lane / VP;
    const int e_mine = grp * EPW + i_env;
    const bool active = e_mine < d.E;
    const int e_ld = active ? e_mine : d.E - 1;
    const int row = e_ld * V + v_mine;
    double2 head[HD ? NCH : 1];
    // the heads gen_head_rank() puts at rank R (-1: this batch), through the same clamped row wherever they are requested
    auto request_heads = [&](auto rc) {
        constexpr int R = decltype(rc)::value;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (gen_head_rank(G, NP, D, c) == R) head[c] = reinterpret_cast<const double2*>(steer)[(long long)row * NCH + c];
    };
    if constexpr (HD) request_heads(std::integral_constant<int, -1>{});
    else head[0].x = steer[row];
    const double2 z = reinterpret_cast<const double2*>(KA.z_r)[row];
    GenIdx<Q> kq;
    float4 tq[TK ? 1 : Q], bq[Q];
    if constexpr (TK) {
        kq = *reinterpret_cast<const GenIdx<Q>*>(A.theta_k + (long long)e_ld * A.theta_k_stride + 2 * Q * v_mine);
    } else {
        const float4* __restrict__ tb = reinterpret_cast<const float4*>(A.theta) + (long long)e_ld * NP + Q * v_mine;
#pragma unroll
        for (int i = 0; i < Q; ++i) tq[i] = tb[i];
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) bq[i] = reinterpret_cast<const float4*>(A.b)[Q * v_mine + i];
    if constexpr (TK) {
        theta_table_fill(s_ph[wave], lane);
        __builtin_amdgcn_wave_barrier();
    }
    // step()'s inputs, and with them -- one scalar round trip -- the arguments the arrival draw reads.  The draw needs
    // nothing from memory: issued here, behind the last request and in front of the wait for the first, it runs while all four
    // wavefronts of the SIMD have nothing else to issue, instead of behind the chains where vector issue is the bound.  The
    // empty asm pins the count here: neither the scheduler nor machine sinking may carry the draw down to its use.
    RISVEC_ARGS_IN_ONE_TRIP("s"(A.action), "s"(A.data_buf), "s"(A.partner), "s"(A.arrivals), "s"(A.n_groups), "s"(A.mec_q),
                            "s"(A.pl), "s"(A.flags), "s"(d.V), "s"(d.env_offset), "s"(A.seed), "s"(A.counter),
                            "s"(KA.P.poisson_cdf[0]), "s"(KA.P.poisson_cdf[1]), "s"(KA.P.poisson_cdf[2]),
                            "s"(KA.P.poisson_cdf[3]), "s"(KA.P.poisson_cdf[4]), "s"(KA.P.poisson_cdf[5]),
                            "s"(KA.P.poisson_cdf[6]), "s"(KA.P.poisson_cdf[7]));
    // (LATE: the draw and its arguments keep this place; the inputs are requested, and held, at the top of leaf IN_RANK)
    In in;
    if constexpr (!LATE) in = Core::load(d, A, e_mine, v_mine, active);
    int arr = Core::draw(d, KA.P, A, e_mine, v_mine);
    asm volatile("" : "+v"(arr));
    if constexpr (!LATE) Core::hold(in);
    if constexpr (TK) ts.mark_behind(kq.w[0], bq[0].x);        // what the first vmcnt wait is for: the lane's theta and b
    else ts.mark_behind(tq[0].x, bq[0].x);

    // the env's w0 / w1 of float4 p, cmul(theta, b) as the reading lane p forms them: Q per lane, shared through s_w
    float4* __restrict__ wrow = s_w[wave] + i_env * WS;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        float2 t0, t1;
        if constexpr (TK) {
            const unsigned k2 = kq.w[i / 2] >> (16 * (i & 1));
            t0 = s_ph[wave][k2 & 15u];
            t1 = s_ph[wave][(k2 >> 8) & 15u];
        } else {
            t0 = make_float2(tq[i].x, tq[i].y);
            t1 = make_float2(tq[i].z, tq[i].w);
        }
        const float2 w0 = cmul(t0, make_float2(bq[i].x, bq[i].y));
        const float2 w1 = cmul(t1, make_float2(bq[i].z, bq[i].w));
        wrow[Q * v_mine + i] = make_float4(w0.x, w0.y, w1.x, w1.y);
    }
    __builtin_amdgcn_wave_barrier();                           // s_w's writes -> its reads (same wave: in order)

    // block J of the partials: float4 gl = 8 J + k of the row, i.e. chunk J (then chunk J + G/8), against w of the same index
    auto leaf = [&](auto jc, float2 (&acc)[8]) {
        constexpr int J = decltype(jc)::value;
        if constexpr (8 * J < NP && ((D > 0 && NL > 1) || LATE)) {
            // Behind the fence of the leaf before (its memory clobber: no request rises above it) and in front of this
            // leaf's chains: step()'s inputs where they are due, then the heads of the leaf D ranks on.  The inputs are
            // held one leaf later, behind that leaf's own requests.  (load_step_in's requests stand under `if (active)`,
            // which the compiler joins with a wait for zero: in fact they are waited for here, with this leaf's head.)
            constexpr int R = gen_leaf_rank(G, NP, J);
            if constexpr (LATE && R == IN_RANK) in = Core::load(d, A, e_mine, v_mine, active);
            if constexpr (D > 0) request_heads(std::integral_constant<int, R>{});
            // Left alone the scheduler sinks the request a hundred instructions into the leaf, behind the wait for this
            // leaf's own head, which is then a wait for zero.  The statement's memory clobber keeps the requests above
            // it, and it reads this leaf's heads, so the wait for them stands behind the requests and counts down to them.
            if constexpr (HD) {
                if constexpr (NIT == 1) asm volatile("" ::"v"(head[J].x), "v"(head[J].y) : "memory");
                else asm volatile("" ::"v"(head[J].x), "v"(head[J].y), "v"(head[J + G / 8].x), "v"(head[J + G / 8].y) : "memory");
            }
            if constexpr (LATE && R == IN_RANK + 1) Core::hold(in);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = make_float2(0.f, 0.f);
        if constexpr (8 * J < NP) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                constexpr int GC = G / 8;
                const int c = J + it * GC;
                float4 q[kGeoChunk / 2];
                if constexpr (HD) steer_chunk_from_head(head[c].x, head[c].y, z.x, z.y, q);
                else steer_chunk(head[0].x, z.x, z.y, c * kGeoChunk, q);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float4 w = wrow[8 * c + k];
                    acc[k] = cfma(make_float2(q[k].x, q[k].y), make_float2(w.x, w.y), acc[k]);
                    acc[k] = cfma(make_float2(q[k].z, q[k].w), make_float2(w.z, w.w), acc[k]);
                }
                // One chain and its 8 float4 of w at a time: left to itself the compiler asks for all of the row's w first
                // (32 float4 in registers at M = 64) and the fourth wavefront per SIMD is lost.  The partials pass through
                // an empty asm that clobbers memory: the next chunk's LDS reads cannot rise above it, nor this chunk's
                // arithmetic sink below it.  The leaf's last fence carries the schedule's change of priority, if it has one
                // there (RISVEC_GEN_FENCE).
                constexpr int level = SCH::prio_change(gen_leaf_rank(G, NP, J) + 1);
                if constexpr (level >= 0) {
                    if (it + 1 == NIT) RISVEC_GEN_FENCE(acc, "s_setprio %[level]", [level] "n"(level));
                    else RISVEC_GEN_FENCE(acc, "", );
                } else {
                    RISVEC_GEN_FENCE(acc, "", );
                }
            }
            ts.mark();                                         // behind the leaf's last fence
        }
    };
    float2 img = row_tree<G>(leaf);
    if constexpr (LATE && IN_RANK + 1 >= NL) Core::hold(in);
    ts.mark_behind(img.x, img.y);                              // row_tree

    const GenArgs<Core>& L = late_args<Core>();
    ts.mark_behind_scalar(L.d.E);                              // one field of the segment back: the wait for late_args()
    Core::template run<VP, GenStores, true>(L.d, L.P, L.A, e_mine, v_mine, active, img, in, arr);
    static_assert(NL + 5 <= kGenStampMax, "entry, first wait, NL leaves, tree, late, end");
    ts.finish(wid, lane, NL + 5);                              // the last store has left
}

// The shapes whose one-group member is the row-per-lane form: those that keep four wavefronts per SIMD (128 VGPRs) with it.
// 16 x 256 does not -- a lane would run 16 chains against 128 float4 of w, 171 ... 204 VGPRs -- and keeps the stage form.
template <int V, int M>
struct GenRowLane {
    static constexpr bool value = M <= 64;
};

template <int V, int M, class Core, bool TK, bool ONE, bool HD>
__global__ void __launch_bounds__(kBlock)
k_step_fused_gen(GenArgs<Core> KA) {
    if constexpr (ONE && GenRowLane<V, M>::value) gen_row_lane_form<V, M, Core, TK, HD>(KA);
    else gen_stage_form<V, M, Core, TK, ONE, HD>(KA);
}

// Wavefronts per CU: no register ring, and 38.5 KiB of LDS per workgroup (the stage), so four workgroups fit a CU.  The
// float64 chain of a pass is long and dependent (one sincospi, 15 rotations): four wavefronts per SIMD cover its
// latency where the reading form's two covered a stream.
constexpr int kGenWavesPerCu = 16;

// risvec_last_gen_groups_per_wave(): the groups per wavefront of the calling thread's last GEN launch
static thread_local int g_gen_per_wave = 0;

template <int V, int M, class Core>
static hipError_t launch_gen(const RisVecState& s, const typename Core::Params& p, const typename Core::Args& a, bool rev,
                             bool heads, hipStream_t st) {
    using S = GenShape<V, M>;
    const int n_groups = (s.n_envs + S::EPW - 1) / S::EPW;
    const int wpb = kBlock / kWave;
    const int forced_waves = forced_forms().pipe_waves;
    long long want_waves = forced_waves > 0 ? forced_waves : (long long)num_cus() * kGenWavesPerCu;
    if (want_waves > n_groups) want_waves = n_groups;
    const long long per_wave = (n_groups + want_waves - 1) / want_waves;
    want_waves = (n_groups + per_wave - 1) / per_wave;
    const unsigned grid = (unsigned)((want_waves + wpb - 1) / wpb);
    const int contiguous = forced_waves > 0 ? (int)per_wave : 0;
    // the heads stand behind the angles in the allocation state.steer_ang points to (RISVEC_STEP_STEER_HEADS_CURRENT)
    const double* steer = heads ? s.steer_ang + (long long)s.n_envs * s.n_veh : s.steer_ang;
    const GenArgs<Core> ka{dims_of(s), p, a, steer, s.z_r, n_groups, contiguous, rev ? 1 : 0};
    auto go = [&](auto knl) { hipLaunchKernelGGL(knl, dim3(grid), dim3(kBlock), 0, st, ka); };
    // one group per wavefront (then the grid covers the groups, whichever way they are dealt): the member without a
    // group loop
    const bool one = per_wave == 1;
    auto pick = [&](auto tk, auto hd) {
        if (one) go(k_step_fused_gen<V, M, Core, decltype(tk)::value, true, decltype(hd)::value>);
        else go(k_step_fused_gen<V, M, Core, decltype(tk)::value, false, decltype(hd)::value>);
    };
    if (a.theta_k != nullptr) {
        if (heads) pick(std::true_type{}, std::true_type{});
        else pick(std::true_type{}, std::false_type{});
    } else {
        if (heads) pick(std::false_type{}, std::true_type{});
        else pick(std::false_type{}, std::false_type{});
    }
    g_gen_per_wave = (int)per_wave;
    return hipGetLastError();
}

int last_gen_launch_groups_per_wave() { return g_gen_per_wave; }

#if RISVEC_GEN_STAMPS
// The stamp buffer of the row-per-lane members: n_waves x kGenStampSlots uint64 of device memory, or nullptr to stop.
// Synchronous; the caller keeps the buffer alive until it has handed over nullptr.
extern "C" int risvec_gen_stamps_buffer(void* buf, long long n_waves) {
    unsigned long long* p = static_cast<unsigned long long*>(buf);
    if (buf == nullptr) n_waves = 0;
    hipError_t err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpyToSymbol(HIP_SYMBOL(g_gen_stamps_waves), &n_waves, sizeof(n_waves));
    if (err == hipSuccess) err = hipMemcpyToSymbol(HIP_SYMBOL(g_gen_stamps), &p, sizeof(p));
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return (int)err;
}
#endif

// the shapes whose rows are whole chunks have GEN members; the others keep reading
template <int V, int M, bool WHOLE = (M % kGeoChunk == 0)>
struct GenMember {
    static hipError_t launch(const RisVecState&, const RisVecParams&, const StepArgs&, bool, bool, bool, hipStream_t) {
        return hipErrorNotSupported;
    }
};
template <int V, int M>
struct GenMember<V, M, true> {
    static hipError_t launch(const RisVecState& s, const RisVecParams& p, const StepArgs& a, bool ring, bool rev, bool heads,
                             hipStream_t st) {
        return ring ? launch_gen<V, M, MarlRingCore<V>>(s, p, a, rev, heads, st)
                    : launch_gen<V, M, MarlCore>(s, p, a, rev, heads, st);
    }
};

hipError_t launch_step_fused_gen(const RisVecState& s, const RisVecParams& p, const StepArgs& a, const StepPlan& pl,
                                 bool rev, bool heads, hipStream_t st) {
    note_pipe_walk(rev ? 1 : 0);
#define RISVEC_X(VV, MM, DD, EMIN, EMAX, T) \
    if (pl.V == VV && pl.M == MM) return GenMember<VV, MM>::launch(s, p, a, pl.ring, rev, heads, st);
    RISVEC_FIXED_SHAPES(RISVEC_X)
#undef RISVEC_X
    return hipErrorNotSupported;
}

// risvec_h_r_from_steer: one thread per chunk, straight to memory
__global__ void __launch_bounds__(kBlock)
k_h_r_from_steer(Dims d, const double* __restrict__ steer_ang, const double* __restrict__ z_r, float* __restrict__ out) {
    const int nchunk = d.M / kGeoChunk;
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)d.E * d.V * nchunk) return;
    const long long ev = idx / nchunk;
    const int m0 = (int)(idx % nchunk) * kGeoChunk;
    const double2 w = reinterpret_cast<const double2*>(z_r)[ev];
    float4 q[kGeoChunk / 2];
    steer_chunk(steer_ang[ev], w.x, w.y, m0, q);
    float4* dst = reinterpret_cast<float4*>(out + (ev * d.M + m0) * 2);
#pragma unroll
    for (int k = 0; k < kGeoChunk / 2; ++k) dst[k] = q[k];
}

// risvec_steer_heads: one thread per chunk, the head as steer_chunk() would start from it
__global__ void __launch_bounds__(kBlock)
k_steer_heads(Dims d, const double* __restrict__ steer_ang, double2* __restrict__ heads) {
    const int nchunk = d.M / kGeoChunk;
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)d.E * d.V * nchunk) return;
    heads[idx] = steer_head(steer_ang[idx / nchunk], (int)(idx % nchunk) * kGeoChunk);
}

hipError_t launch_steer_heads(const RisVecState& s, double* heads, hipStream_t st) {
    const long long n = (long long)s.n_envs * s.n_veh * (s.n_ris / kGeoChunk);
    hipLaunchKernelGGL(k_steer_heads, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dims_of(s), s.steer_ang,
                       reinterpret_cast<double2*>(heads));
    return hipGetLastError();
}

hipError_t launch_h_r_from_steer(const RisVecState& s, float* out, hipStream_t st) {
    const long long n = (long long)s.n_envs * s.n_veh * (s.n_ris / kGeoChunk);
    hipLaunchKernelGGL(k_h_r_from_steer, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dims_of(s),
                       s.steer_ang, s.z_r, out);
    return hipGetLastError();
}

}  // namespace risvec
