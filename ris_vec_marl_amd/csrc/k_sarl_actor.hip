// The single-agent (DDPG) actor, ActorNetwork.forward (Simulation-SARL/networks.py:132-141), in ONE kernel:
// fc1 -> LayerNorm -> ReLU -> fc2 -> LayerNorm -> ReLU -> mu -> sigmoid for n_rows rows that share ONE weight set, every
// product on the fp16 matrix cores at float32 accuracy and neither hidden layer ever written to memory.
//
// Orientation, precision and register order are those of risvec_mfma.hpp (read its header): a wavefront owns 32 rows, a
// lane holds its row's features in registers, and each layer's output is the next MFMA's B operand as it stands.
//
// What differs from k_policy_mlp:
//  * fc1 has 80+ inputs, so it is a real MFMA product (K = in_dims + 1 padded to KS k-steps of 16: the bias is one more
//    input row at x = 1), with the observation held in registers as the split B operand, and LayerNorm-1 takes TWO
//    passes over the fc1 weight.  The weight is centred over the feature axis on the host, so the pre-activation has
//    mean 0 and its variance is a plain sum of squares: pass 1 accumulates it group by group (32 features), pass 2
//    recomputes each group (bit-identically), normalises, applies the ReLU, splits and feeds fc2 at once.  No LDS for
//    activations, and the 4 MT fc2 accumulators stay the only large register block.
//  * one weight set for all rows: ONE stream of fixed-size ITEMS (R fragment rows of 1 KiB = 64 lanes x 8 halfs), read
//    L2 -> LDS by LDS-direct loads into a ring of three slots, two items ahead of the MFMAs, with counted
//    s_waitcnt vmcnt + raw s_barrier as in k_policy_mlp.  Items in stream order:
//      T1 pass-1 items   P1 = R / (2 KS) groups each; group i at rows 2 KS i: row 2 s + t = fragment (k-step s, t = hi / lo)
//      NG pass-2 items   one group each: rows [0, 2 KS) its fc1 fragments again, row 2 KS its LayerNorm-1 weight [32] and
//                        bias [32] as float32, rows 2 KS + 1 .. : the two fc2 chunks [u][hi|lo][m] of k_policy_mlp
//      TH head items     HS = R / (2 HT) k-steps each (HT = ceil(n_actions / 32) output tiles): k-step j of the item at
//                        rows 2 HT j, row 2 ht + t
//    Every item is R rows whatever it holds, so every stage is the same number of loads per lane and the counted waits
//    are compile-time constants.
//  * workgroup = 4 wavefronts (one per SIMD, 128 rows): 32 768 rows are 256 workgroups, one per CU; the ring
//    (3 R KiB, up to 156 KiB) is the whole LDS footprint -- the fc2 / head parameters are read from global memory once.
//
// Every s_barrier sits under wave-uniform control flow: all loop bounds come from kernel arguments and template
// parameters, and rows at or beyond n_rows are computed on row 0's input and never stored.
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"
#include "risvec_step.hpp"

namespace risvec {
namespace {

struct ActorArgs {
    long long n_rows;
    int IN, NG, A, HT, T1, T;
    const float* x;          // [n_rows, IN]
    const uint4* ws;         // [T, R, 64] 16-byte fragments: the weight stream
    const float* scales;     // [3] undo the fc1, fc2 and head weight scalings
    const float* b2; const float* ln2w; const float* ln2b;   // [F2]
    const float* bmu;        // [A]
    float* logits;           // [n_rows, A] or NULL
    float* mu;               // [n_rows, A]
};

constexpr int kActBlock = 256;       // 4 wavefronts = 1 per SIMD
constexpr int kRing = 3;             // item slots in LDS: one being read, two in flight / landed
constexpr int kMaxHT = 3;            // n_actions <= 96

constexpr int actor_rows(int MT, int KS) { return (2 * KS + 1 + 4 * MT + 3) & ~3; }

template <int MT, int KS>
__global__ void __launch_bounds__(kActBlock)
k_sarl_actor(ActorArgs A) {
    constexpr int F2 = 32 * MT;
    constexpr int kRows = actor_rows(MT, KS);
    constexpr int kSlotVec = kRows * kWave;                   // uint4 per item
    constexpr int kStage = kSlotVec / kActBlock;              // LDS-direct loads per lane per item
    static_assert(kSlotVec % kActBlock == 0, "item must split evenly over the workgroup");
    static_assert(2 * kStage < 60, "two items in flight must fit the vmcnt counter");
    constexpr int kP1 = kRows / (2 * KS);                     // groups per pass-1 item
    constexpr int kChunkVec = 2 * MT * kWave;                 // uint4 per fc2 chunk of 16 hidden features
    constexpr int kF2Vec = (2 * KS + 1) * kWave;              // where the fc2 chunks start in a pass-2 item
    extern __shared__ uint4 s_ring[];                         // [kRing][kSlotVec]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int NG = A.NG, T = A.T, HT = A.HT;
    auto stage = [&](int t) {                                 // item t of the weight stream, global -> LDS directly
        const uint4* src = A.ws + (size_t)t * kSlotVec;
        uint4* dst = s_ring + (t % kRing) * kSlotVec;
#pragma unroll
        for (int q = 0; q < kStage; ++q)
            __builtin_amdgcn_global_load_lds((const gvoid_t*)(src + q * kActBlock + tid), (lvoid_t*)(dst + q * kActBlock + tid), 16, 0, 0);
    };
    // item t is done with: item t+1 has landed for every wavefront, item t+2 (if any) stays in flight across the barrier.
    // Raw s_barrier: __syncthreads() would drain the LDS-direct loads (vmcnt(0)).
    auto end_item = [&](int t) {
        if (t + 2 < T) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kStage) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    stage(0);
    stage(1);                                                 // T >= 3: there is at least one item of each kind
    const float u1 = A.scales[0], u2 = A.scales[1], uh = A.scales[2];   // requested here: a later global load would have
                                                              // to drain the weight stream (vmcnt retires in order)

    // this lane's row as the split B operand of fc1: k-step s holds x[16 s + 8 h + j], j < 8; x[IN] = 1 (the bias row)
    const long long e = ((long long)blockIdx.x * (kActBlock / kWave) + wave) * 32 + r;
    const int IN = A.IN;
    half8_t xh[KS], xl[KS];
    {
        const float* xin = A.x + (e < A.n_rows ? e : 0) * IN;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            f32x8_t xb;
            if ((IN & 3) == 0) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k0 = 16 * s + 8 * h + 4 * c;
                    float4 v = make_float4(k0 == IN ? 1.0f : 0.0f, 0.0f, 0.0f, 0.0f);
                    if (k0 < IN) v = *reinterpret_cast<const float4*>(xin + k0);
                    xb[4 * c] = v.x; xb[4 * c + 1] = v.y; xb[4 * c + 2] = v.z; xb[4 * c + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * h + j;
                    xb[j] = k < IN ? xin[k] : (k == IN ? 1.0f : 0.0f);
                }
            }
            split16(xb, xh[s], xl[s]);
        }
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kStage) : "memory");   // item 0 has landed (item 1 was issued after it)
    __builtin_amdgcn_s_barrier();

    // The scaled, centred fc1 pre-activation of 32 features of this lane's row, C/D layout; w1 = the group's 2 KS
    // fragment rows.  The A fragments are read one k-step ahead by hand (see mfma_chunk).
    auto fc1_tile = [&](const uint4* w1) {
        const uint32_t base = (uint32_t)(size_t)(lvoid_t*)(w1 + lane);
        half8_t fh[2], fl[2];
        f32x16_t d;
#pragma unroll
        for (int q = 0; q < 16; ++q) d[q] = 0.0f;
#define RISVEC_RD1(S_) do {                                                                                  \
            asm volatile("ds_read_b128 %0, %1" : "=v"(fh[(S_) & 1]) : "v"(base + (2 * (S_)) * kWave * 16));        \
            asm volatile("ds_read_b128 %0, %1" : "=v"(fl[(S_) & 1]) : "v"(base + (2 * (S_) + 1) * kWave * 16));    \
        } while (0)
        RISVEC_RD1(0);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (s + 1 < KS) {
                RISVEC_RD1(s + 1);
                asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(fh[s & 1]), "+v"(fl[s & 1]));
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fh[s & 1]), "+v"(fl[s & 1]));
            }
            d = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[s & 1], xh[s], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl[s & 1], xh[s], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh[s & 1], xl[s], d, 0, 0, 0);
        }
#undef RISVEC_RD1
        return d;
    };

    // ---- pass 1: LayerNorm-1 variance = sum over all fc1 features of the squared centred pre-activation
    float ss = 0.0f;
    int t = 0;
    for (; t < A.T1; ++t) {
        const uint4* slot = s_ring + (t % kRing) * kSlotVec;
        if (t + 2 < T) stage(t + 2);
        const int left = NG - t * kP1, ng = left < kP1 ? left : kP1;
        for (int i = 0; i < ng; ++i) {
            const f32x16_t d = fc1_tile(slot + i * (2 * KS * kWave));
            const f32x16_t d2 = d * d;
#pragma unroll
            for (int q = 0; q < 16; ++q) ss += d2[q];
        }
        end_item(t);
    }
    ss += __shfl_xor(ss, 32, kWave);
    const float k1 = rsqrtf((ss * u1) * u1 / (float)(32 * NG) + kLnEps) * u1;   // rstd, with the weight scaling undone

    // ---- pass 2: fc1 group -> LayerNorm-1 + ReLU -> split -> fc2, accumulated over the groups
    f32x16_t acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
    // registers 8u .. 8u+7 of a C/D tile -> the split B fragments of k-step u
    auto make_b = [&](const f32x16_t& y, int u, half8_t (&bf)[2]) {
        f32x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = y[8 * u + j];
        split16(v, bf[0], bf[1]);
    };
    // k_policy_mlp.hip's mfma_chunk and its reasons, word for word (lifting it into risvec_mfma.hpp changes the schedule)
    auto mfma_chunk = [&](const uint4* sa, const half8_t (&bf)[2]) {
        const uint32_t base = (uint32_t)(size_t)(lvoid_t*)(sa + lane);
        half8_t ah[3], al[3];
#define RISVEC_RD(M_) do {                                                                                          \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ah[(M_) % 3]) : "v"(base), "n"((M_) * kWave * 16));          \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(al[(M_) % 3]) : "v"(base), "n"((MT + (M_)) * kWave * 16));   \
        } while (0)
        RISVEC_RD(0);
        if constexpr (MT > 1) RISVEC_RD(1);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m + 2 < MT) {
                if (m == 0) RISVEC_RD(2); else if (m == 1) RISVEC_RD(3); else if (m == 2) RISVEC_RD(4);
                else if (m == 3) RISVEC_RD(5); else if (m == 4) RISVEC_RD(6); else RISVEC_RD(7);
                asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(ah[m % 3]), "+v"(al[m % 3]));
            } else if (m + 1 < MT) {
                asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(ah[m % 3]), "+v"(al[m % 3]));
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ah[m % 3]), "+v"(al[m % 3]));
            }
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m % 3], bf[0], acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m % 3], bf[0], acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m % 3], bf[1], acc[m], 0, 0, 0);
        }
#undef RISVEC_RD
    };
    for (int g = 0; g < NG; ++g, ++t) {
        const uint4* slot = s_ring + (t % kRing) * kSlotVec;
        if (t + 2 < T) stage(t + 2);
        // LayerNorm-1 weight [32] and bias [32] of the group, requested in front of the fc1 fragments.  Every LDS read of
        // the ring is inline asm: a compiler-generated ds_read makes hipcc drain the LDS-direct loads first (vmcnt(0)).
        const uint32_t lp = (uint32_t)(size_t)(lvoid_t*)(slot + 2 * KS * kWave) + 16 * h;
        f32x4_t w4[4], b4[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(w4[gq]) : "v"(lp + 32 * gq));
            asm volatile("ds_read_b128 %0, %1" : "=v"(b4[gq]) : "v"(lp + 128 + 32 * gq));
        }
        const f32x16_t d = fc1_tile(slot);                       // ends on lgkmcnt(0): the eight reads above are in
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w4[0]), "+v"(w4[1]), "+v"(w4[2]), "+v"(w4[3]), "+v"(b4[0]), "+v"(b4[1]),
                     "+v"(b4[2]), "+v"(b4[3]));
        f32x16_t y;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * gq + i] = fmaxf(fmaf(d[4 * gq + i] * k1, w4[gq][i], b4[gq][i]), 0.0f);
        half8_t b0[2], b1[2];
        make_b(y, 0, b0);
        mfma_chunk(slot + kF2Vec, b0);
        make_b(y, 1, b1);
        mfma_chunk(slot + kF2Vec + kChunkVec, b1);
        end_item(t);
    }

    // ---- fc2 bias + LayerNorm + ReLU, in registers: this lane owns features 32m + (q & 3) + 8 (q >> 2) + 4h of its row
    // (the twin of the block in k_policy_mlp.hip; keep the two in step)
    const float inv_f2 = 1.0f / (float)F2;
    {
        auto tile_of = [&](const float* tab, int m) {            // 16 per-feature parameters in C/D register order
            f32x16_t tl;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 q4 = *reinterpret_cast<const float4*>(tab + 32 * m + 8 * g + 4 * h);
                tl[4 * g] = q4.x; tl[4 * g + 1] = q4.y; tl[4 * g + 2] = q4.z; tl[4 * g + 3] = q4.w;
            }
            return tl;
        };
        f32x16_t vs;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc[m] = acc[m] * u2 + tile_of(A.b2, m);
            vs = m == 0 ? acc[0] : vs + acc[m];
        }
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += vs[q];
        s += __shfl_xor(s, 32, kWave);
        const float mean = s * inv_f2;
        f32x16_t v2;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc[m] = acc[m] - mean;                               // centred once, reused by the normalisation
            v2 = m == 0 ? acc[0] * acc[0] : v2 + acc[m] * acc[m];
        }
        float s2 = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s2 += v2[q];
        s2 += __shfl_xor(s2, 32, kWave);
        const float rs = rsqrtf(s2 * inv_f2 + kLnEps);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc[m] = (acc[m] * rs) * tile_of(A.ln2w, m) + tile_of(A.ln2b, m);
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][q] = fmaxf(acc[m][q], 0.0f);
        }
    }

    // ---- the head on the matrix cores: D[action][row] = Wmu . y with the accumulator registers themselves as the B
    // operand (registers 8u .. 8u+7 of tile m are k-step 2m + u), HT output tiles, HS k-steps per item
    f32x16_t hacc[kMaxHT];
#pragma unroll
    for (int ht = 0; ht < kMaxHT; ++ht)
#pragma unroll
        for (int q = 0; q < 16; ++q) hacc[ht][q] = 0.0f;
    {
        const int HS = kRows / (2 * HT);
        const uint4* slot = s_ring + (t % kRing) * kSlotVec;
        if (t + 2 < T) stage(t + 2);
        int jj = 0;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (jj == HS) {                                   // wave-uniform: HS comes from the arguments
                    end_item(t);
                    ++t;
                    slot = s_ring + (t % kRing) * kSlotVec;
                    if (t + 2 < T) stage(t + 2);
                    jj = 0;
                }
                const uint32_t wr = (uint32_t)(size_t)(lvoid_t*)(slot + (jj * HT * 2) * kWave + lane);
                half8_t wh[kMaxHT], wl[kMaxHT];
#pragma unroll
                for (int ht = 0; ht < kMaxHT; ++ht)
                    if (ht < HT) {
                        asm volatile("ds_read_b128 %0, %1" : "=v"(wh[ht]) : "v"(wr + (2 * ht) * kWave * 16));
                        asm volatile("ds_read_b128 %0, %1" : "=v"(wl[ht]) : "v"(wr + (2 * ht + 1) * kWave * 16));
                    }
                half8_t yb[2];
                make_b(acc[m], u, yb);                            // behind the reads
#pragma unroll
                for (int ht = 0; ht < kMaxHT; ++ht)
                    if (ht < HT) {
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wh[ht]), "+v"(wl[ht]));
                        hacc[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ht], yb[0], hacc[ht], 0, 0, 0);
                        hacc[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[ht], yb[0], hacc[ht], 0, 0, 0);
                        hacc[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ht], yb[1], hacc[ht], 0, 0, 0);
                    }
                ++jj;
            }
        end_item(t);
    }

    // actions 32 ht + (q & 3) + 8 (q >> 2) + 4h: four groups of four consecutive actions per lane and tile
    const int NA = A.A;
    const bool vec4 = (NA & 3) == 0;
#pragma unroll
    for (int ht = 0; ht < kMaxHT; ++ht)
        if (ht < HT) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int a0 = 32 * ht + 8 * gq + 4 * h;
                float lg[4], sg[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    lg[k] = fmaf(hacc[ht][4 * gq + k], uh, a0 + k < NA ? A.bmu[a0 + k] : 0.0f);
                    sg[k] = 1.0f / (1.0f + expf(-lg[k]));
                }
                if (e < A.n_rows && a0 < NA) {
                    const size_t o = (size_t)e * NA + a0;
                    if (vec4) {
                        *reinterpret_cast<float4*>(A.mu + o) = make_float4(sg[0], sg[1], sg[2], sg[3]);
                        if (A.logits) *reinterpret_cast<float4*>(A.logits + o) = make_float4(lg[0], lg[1], lg[2], lg[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (a0 + k < NA) {
                                A.mu[o + k] = sg[k];
                                if (A.logits) A.logits[o + k] = lg[k];
                            }
                    }
                }
            }
        }
}

// the fc1 k-step counts the kernel is built for: in_dims + 1 (the bias row) is padded up to the next of them
constexpr int kKs[4] = {3, 6, 7, 9};

int ks_built(int IN) {
    const int ks = ks_of(IN + 1);
    for (int k : kKs)
        if (ks <= k) return k;
    return 0;
}

template <int MT, int KS>
hipError_t launch_actor(const ActorArgs& a, hipStream_t st) {
    const size_t lds = (size_t)kRing * actor_rows(MT, KS) * kWave * sizeof(uint4);
    const long long rows = (kActBlock / kWave) * 32;
    return launch_dynamic_lds(k_sarl_actor<MT, KS>, dim3((unsigned)((a.n_rows + rows - 1) / rows)), dim3(kActBlock), lds, st, a);
}

template <int MT>
hipError_t launch_actor_ks(int ks, const ActorArgs& a, hipStream_t st) {
    switch (ks) {
        case 3: return launch_actor<MT, 3>(a, st);
        case 6: return launch_actor<MT, 6>(a, st);
        case 7: return launch_actor<MT, 7>(a, st);
        case 9: return launch_actor<MT, 9>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace

bool sarl_actor_supported(int IN, int F1, int F2, int A) {
    return IN >= 1 && IN <= 128 && F1 >= 32 && F1 % 32 == 0 && F1 <= 1024 && (F2 == 256 || F2 == 128) && A >= 1 && A <= 32 * kMaxHT;
}

SarlActorGeom sarl_actor_geom(int IN, int F1, int F2, int A) {
    SarlActorGeom g{};
    if (!sarl_actor_supported(IN, F1, F2, A)) return g;
    g.ks = ks_built(IN);
    g.mt = F2 / 32;
    g.ht = (A + 31) / 32;
    g.ng = F1 / 32;
    g.rows = actor_rows(g.mt, g.ks);
    const int p1 = g.rows / (2 * g.ks), hs = g.rows / (2 * g.ht);
    g.t1 = (g.ng + p1 - 1) / p1;
    g.th = (2 * g.mt + hs - 1) / hs;
    g.items = g.t1 + g.ng + g.th;
    g.stream_bytes = (long long)g.items * g.rows * kWave * (long long)sizeof(uint4);
    return g;
}

hipError_t launch_sarl_actor(long long n_rows, int IN, int F1, int F2, int A, const float* x, const void* wstream,
                             const float* scales, const float* b2, const float* ln2w, const float* ln2b, const float* bmu,
                             float* logits, float* mu, hipStream_t st) {
    const SarlActorGeom g = sarl_actor_geom(IN, F1, F2, A);
    if (g.items == 0) return hipErrorInvalidValue;
    ActorArgs a{n_rows, IN, g.ng, A, g.ht, g.t1, g.items, x, static_cast<const uint4*>(wstream), scales, b2, ln2w, ln2b, bmu,
                logits, mu};
    note_kernel("k_sarl_actor<%d,%d>", g.mt, g.ks);
    return F2 == 256 ? launch_actor_ks<8>(g.ks, a, st) : launch_actor_ks<4>(g.ks, a, st);
}

}  // namespace risvec
