// The single-agent (DDPG) critic, CriticNetwork.forward (Simulation-SARL/networks.py:66-79), and the TD target of
// learn() (ddpg_torch.py:84-88) in ONE kernel, for n_rows rows that share ONE weight set:
//     s = relu(LN1(fc1 x));  s = LN2(fc2 s);  h = relu(s + action_value(a));  h = relu(LN3(fc3 h));  q = q_w . h + q_b
//     y = done ? reward : reward + gamma q
// Orientation, precision and register order are those of risvec_mfma.hpp (read its header).  fc1 is centred over the
// feature axis on the host with the bias as one more input row at x = 1, so LayerNorm-1's mean is 0 and its variance a
// plain sum of squares.
//
// What differs from k_sarl_actor -- the FORM.  The actor holds 32 rows and every fc2 accumulator in one wavefront
// (256 VGPRs + 202 AGPRs at fc2 = 256); fc2 = 512 plus an fc3 block does not fit that.  Here a workgroup of four
// wavefronts shares ONE tile of 32 rows and splits the OUTPUT FEATURES of every layer four ways: wavefront w owns fc1
// groups w, w + 4, .. and output tiles [w MT, (w + 1) MT) of fc2 / action_value / fc3 (MT = features / 128).  A weight
// fragment is therefore used by exactly one wavefront of the workgroup, so it goes L2 -> registers with plain global
// loads, four k-steps ahead of its MFMAs (no LDS staging: nothing would share it), and LDS holds what IS shared:
//   s_in  the split B fragments of the input x                         [KS k-steps][hi | lo][64 lanes] x 16 bytes
//   s_h   first those of the action, then the fc1 activations, then the fc2 activations (each dead before the next)
//   s_red the per-row partial sums of the three LayerNorms and of the q dot product, one slot per use: [6][4 waves][32]
// A lane leaves its C/D tile in LDS as two k-steps (registers 8u .. 8u+7 = k-step u, the permuted k order of the actor)
// and every wavefront reads them back as B operands with one ds_read_b128 per fragment.  LayerNorm-1 takes one fc1
// pass: the raw pre-activation waits in the 64 bytes of LDS that its own split fragments replace after the variance
// is known (lane-private, same bytes).
//
// The fc1 group walk (critic_fc1_walk, with the LayerNorm-1 statistics as its per-group callback), the input-fragment
// store (put_input) and the s_red reduction (marl_red) are risvec_critic_walk.hpp's, shared with the multi-agent critic
// kernels.  LayerNorm, the action branch and the s_red slot count (kSarlRedSlots) are this kernel's own.
//
// Every barrier sits under wave-uniform control flow: all loop bounds come from kernel arguments, template parameters
// and the wavefront index.  Rows at or beyond n_rows are computed on row 0's input and never stored.  No global
// address depends on loaded data; every weight prefetch index is clamped to the last fragment of its block.
#include "risvec_critic_walk.hpp"
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"
#include "risvec_step.hpp"

namespace risvec {
namespace {

struct CriticArgs {
    long long n_rows;
    int IN, NA, KS, KSA, NG;       // NG = fc1 / 32; KS / KSA = k-steps of 16 of [x ; 1] and of a
    const float* x;                // [n_rows, IN]
    const float* a;                // [n_rows, NA]
    const uint4* ws;               // the weight stream: fragment rows of 64 x 16 bytes
    const float* scales;           // [4] undo the fc1, fc2, action_value and fc3 weight scalings
    const float* ln1w; const float* ln1b;                                          // [F1]
    const float* b2; const float* ln2w; const float* ln2b; const float* bav;       // [F2]
    const float* b3; const float* ln3w; const float* ln3b; const float* qw;        // [F3]
    const float* qb;               // [1]
    const float* reward;           // [n_rows] or NULL
    const uint8_t* done;           // [n_rows] or NULL
    float gamma;
    float* q;                      // [n_rows] or NULL
    float* y;                      // [n_rows] or NULL
};

constexpr int kCrBlock = kMcBlock;   // the walk's workgroup: 4 wavefronts = 1 per SIMD, all on the same 32 rows
constexpr int kSarlRedSlots = 6;     // s_red slots: three LayerNorms (variance; mean, variance; mean, variance) and q

template <int MT2, int MT3>
__global__ void __launch_bounds__(kCrBlock)
k_sarl_critic(CriticArgs A) {
    constexpr int F2 = 32 * MT2 * kCriticWaves, F3 = 32 * MT3 * kCriticWaves;
    constexpr int K3 = F2 / 16;                                // fc3 k-steps
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int KS = A.KS, KSA = A.KSA, NG = A.NG;
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(KSA, 2 NG, K3)][2][64]
    const int hsteps = max(max(KSA, 2 * NG), K3);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kSarlRedSlots][4][32]
    const CriticLayout L = critic_layout(KS, KSA, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32;
    const float u1 = A.scales[0], u2 = A.scales[1], uav = A.scales[2], u3 = A.scales[3];

    // ---- the inputs as split B fragments: k-step s, lane (r, h) holds v[16 s + 8 h + j], j < 8; x[IN] = 1 (the bias row)
    auto stage_in = [&](const float* src, int W, int ks, bool one, uint4* dst) {
        for (int idx = tid; idx < ks * kWave; idx += kCrBlock) {
            const int s = idx >> 6, l = idx & 63, rr = l & 31, hh = l >> 5;
            const long long row = e0 + rr < A.n_rows ? e0 + rr : 0;
            const float* p = src + row * W;
            f32x8_t v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * hh + j;
                v[j] = k < W ? p[k] : (one && k == W ? 1.0f : 0.0f);
            }
            put_input(dst, s, l, v);
        }
    };
    stage_in(A.x, A.IN, KS, true, s_in);
    stage_in(A.a, A.NA, KSA, false, s_h);
    __syncthreads();

    // ---- action_value(a): this wavefront's MT2 output tiles, kept until the add
    f32x16_t av[MT2];
#pragma unroll
    for (int m = 0; m < MT2; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) av[m][q] = 0.0f;
    gemm_tiles<MT2>(av, A.ws + (L.av + (long long)wave * KSA * MT2 * 2) * kWave, s_h, KSA, lane);
    __syncthreads();                                          // the action fragments are dead: s_h takes fc1

    // ---- fc1 (the group walk of risvec_critic_walk.hpp): the scaled, centred pre-activation goes to LDS raw (float32, in the
    // 64 bytes per lane that its split fragments will occupy), its squares into the LayerNorm-1 variance
    auto own_slot = [&](int g, int c) { return s_h + ((2 * g) * 2 + c) * kWave + lane; };   // c < 4: (u, t) = (c >> 1, c & 1)
    float ss = 0.0f;
    critic_fc1_walk(A.ws + L.fc1 * kWave, s_in, KS, NG, wave, lane, [&](int g, const f32x16_t& d) {
        ss += sum16(d * d);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float4 v = make_float4(d[4 * c], d[4 * c + 1], d[4 * c + 2], d[4 * c + 3]);
            *reinterpret_cast<float4*>(own_slot(g, c)) = v;
        }
    });
    ss += __shfl_xor(ss, 32, kWave);
    if (h == 0) s_red[(0 * kCriticWaves + wave) * 32 + r] = ss;
    __syncthreads();
    auto red = [&](int slot) { return marl_red(s_red, slot, r); };
    {
        const float k1 = rsqrtf((red(0) * u1) * u1 / (float)(32 * NG) + kLnEps) * u1;   // rstd, the weight scaling undone
        for (int g = wave; g < NG; g += kCriticWaves) {
            f32x16_t d;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(own_slot(g, c));
                d[4 * c] = v.x; d[4 * c + 1] = v.y; d[4 * c + 2] = v.z; d[4 * c + 3] = v.w;
            }
            const f32x16_t w = tile_of(A.ln1w, 32 * g, h), b = tile_of(A.ln1b, 32 * g, h);
            f32x16_t y;
#pragma unroll
            for (int q = 0; q < 16; ++q) y[q] = fmaxf(fmaf(d[q] * k1, w[q], b[q]), 0.0f);
            put_tile(s_h, g, y, lane);
        }
    }
    __syncthreads();

    // ---- fc2: output tiles [wave MT2, (wave + 1) MT2) over all 2 NG k-steps, then LayerNorm-2 across the four wavefronts
    f32x16_t acc[MT2];
#pragma unroll
    for (int m = 0; m < MT2; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
    gemm_tiles<MT2>(acc, A.ws + (L.fc2 + (long long)wave * (2 * NG) * MT2 * 2) * kWave, s_h, 2 * NG, lane);
    {
        f32x16_t vs;
#pragma unroll
        for (int m = 0; m < MT2; ++m) {
            acc[m] = acc[m] * u2 + tile_of(A.b2, 32 * (wave * MT2 + m), h);
            vs = m == 0 ? acc[0] : vs + acc[m];
        }
        float s = sum16(vs);
        s += __shfl_xor(s, 32, kWave);
        if (h == 0) s_red[(1 * kCriticWaves + wave) * 32 + r] = s;
        __syncthreads();                                      // every wavefront is past its fc2 MFMAs: s_h is free
        const float mean = red(1) * (1.0f / (float)F2);
        f32x16_t v2;
#pragma unroll
        for (int m = 0; m < MT2; ++m) {
            acc[m] = acc[m] - mean;
            v2 = m == 0 ? acc[0] * acc[0] : v2 + acc[m] * acc[m];
        }
        float s2 = sum16(v2);
        s2 += __shfl_xor(s2, 32, kWave);
        if (h == 0) s_red[(2 * kCriticWaves + wave) * 32 + r] = s2;
        __syncthreads();
        const float rs = rsqrtf(red(2) * (1.0f / (float)F2) + kLnEps);
#pragma unroll
        for (int m = 0; m < MT2; ++m) {
            const int f0 = 32 * (wave * MT2 + m);
            f32x16_t y = (acc[m] * rs) * tile_of(A.ln2w, f0, h) + tile_of(A.ln2b, f0, h);
            y = y + (av[m] * uav + tile_of(A.bav, f0, h));
#pragma unroll
            for (int q = 0; q < 16; ++q) y[q] = fmaxf(y[q], 0.0f);
            put_tile(s_h, wave * MT2 + m, y, lane);
        }
    }
    __syncthreads();

    // ---- fc3 + LayerNorm-3 + ReLU, then the 1-wide q layer as a dot product in registers
    f32x16_t a3[MT3];
#pragma unroll
    for (int m = 0; m < MT3; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) a3[m][q] = 0.0f;
    gemm_tiles<MT3>(a3, A.ws + (L.fc3 + (long long)wave * K3 * MT3 * 2) * kWave, s_h, K3, lane);
    {
        f32x16_t vs;
#pragma unroll
        for (int m = 0; m < MT3; ++m) {
            a3[m] = a3[m] * u3 + tile_of(A.b3, 32 * (wave * MT3 + m), h);
            vs = m == 0 ? a3[0] : vs + a3[m];
        }
        float s = sum16(vs);
        s += __shfl_xor(s, 32, kWave);
        if (h == 0) s_red[(3 * kCriticWaves + wave) * 32 + r] = s;
        __syncthreads();
        const float mean = red(3) * (1.0f / (float)F3);
        f32x16_t v2;
#pragma unroll
        for (int m = 0; m < MT3; ++m) {
            a3[m] = a3[m] - mean;
            v2 = m == 0 ? a3[0] * a3[0] : v2 + a3[m] * a3[m];
        }
        float s2 = sum16(v2);
        s2 += __shfl_xor(s2, 32, kWave);
        if (h == 0) s_red[(4 * kCriticWaves + wave) * 32 + r] = s2;
        __syncthreads();
        const float rs = rsqrtf(red(4) * (1.0f / (float)F3) + kLnEps);
        f32x16_t qs;
#pragma unroll
        for (int m = 0; m < MT3; ++m) {
            const int f0 = 32 * (wave * MT3 + m);
            f32x16_t y = (a3[m] * rs) * tile_of(A.ln3w, f0, h) + tile_of(A.ln3b, f0, h);
#pragma unroll
            for (int q = 0; q < 16; ++q) y[q] = fmaxf(y[q], 0.0f);
            const f32x16_t p = y * tile_of(A.qw, f0, h);
            qs = m == 0 ? p : qs + p;
        }
        float qp = sum16(qs);
        qp += __shfl_xor(qp, 32, kWave);
        if (h == 0) s_red[(5 * kCriticWaves + wave) * 32 + r] = qp;
        __syncthreads();
    }
    if (wave == 0 && h == 0) {
        const long long e = e0 + r;
        if (e < A.n_rows) {
            const float qv = red(5) + A.qb[0];
            if (A.q) A.q[e] = qv;
            if (A.y) {
                const float rw = A.reward[e];
                A.y[e] = A.done[e] ? rw : fmaf(A.gamma, qv, rw);     // a select, as critic_value_[done] = 0.0 is
            }
        }
    }
}

template <int MT2, int MT3>
hipError_t launch_critic(const CriticArgs& a, hipStream_t st) {
    const int hsteps = std::max(std::max(a.KSA, 2 * a.NG), 8 * MT2);
    const size_t lds = (size_t)(a.KS + hsteps) * 2 * kWave * sizeof(uint4) + (size_t)kSarlRedSlots * kCriticWaves * 32 * sizeof(float);
    return launch_dynamic_lds(k_sarl_critic<MT2, MT3>, dim3((unsigned)((a.n_rows + 31) / 32)), dim3(kCrBlock), lds, st, a);
}

}  // namespace

bool sarl_critic_supported(int IN, int F1, int F2, int F3, int A) {
    return IN >= 1 && IN <= 128 && F1 >= 32 && F1 % 32 == 0 && F1 <= 1024 && (F2 == 128 || F2 == 256 || F2 == 512) &&
           (F3 == 128 || F3 == 256) && A >= 1 && A <= 96;
}

long long sarl_critic_stream_bytes(int IN, int F1, int F2, int F3, int A) {
    if (!sarl_critic_supported(IN, F1, F2, F3, A)) return 0;
    return critic_layout(ks_of(IN + 1), ks_of(A), F1 / 32, F2 / 128, F3 / 128).rows * kWave * (long long)sizeof(uint4);
}

hipError_t launch_sarl_critic(long long n_rows, int IN, int F1, int F2, int F3, int A, const float* x, const float* a,
                              const void* wstream, const float* scales, const float* ln1w, const float* ln1b, const float* b2,
                              const float* ln2w, const float* ln2b, const float* bav, const float* b3, const float* ln3w,
                              const float* ln3b, const float* qw, const float* qb, const float* reward, const uint8_t* done,
                              float gamma, float* q, float* y, hipStream_t st) {
    if (!sarl_critic_supported(IN, F1, F2, F3, A)) return hipErrorInvalidValue;
    CriticArgs c{n_rows, IN, A, ks_of(IN + 1), ks_of(A), F1 / 32, x, a, static_cast<const uint4*>(wstream), scales, ln1w, ln1b,
                 b2, ln2w, ln2b, bav, b3, ln3w, ln3b, qw, qb, reward, done, gamma, q, y};
    note_kernel("k_sarl_critic<%d,%d>", F2 / 128, F3 / 128);
    return dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) { return launch_critic<decltype(mt2)::value, decltype(mt3)::value>(c, st); });
}

}  // namespace risvec
