// The weight stream of k_sarl_critic.hip, built on the device from the float32 weights in two launches: what
// pack_critic_weights (ris_vec_marl_amd/critic.py) computes with library kernels, element for element.
//
//   k_sarl_critic_pack_stats  1 + kMaxBlocks workgroups that never talk to each other.  Workgroup 0 does what needs one
//                             fixed order: the float64 mean over the fc1 features of every row of [W1^T ; b1] (the sum
//                             order of k_sarl_actor_pack_stats: 16 wavefronts, then their partial sums in wavefront
//                             order) and the largest magnitude of the centred fc1 operand; both go to the workspace.
//                             Workgroup 1 + b takes slice b of W2, of Wav and of W3 and leaves the largest magnitude of
//                             each in slot b of the workspace.  A maximum does not depend on the order it is taken in, a
//                             slot has one writer, every slot is written: no atomics, no counters, nothing to initialise.
//   k_sarl_critic_pack        one lane per PAIR of 16-byte fragments: the hi and the lo fragment of the same 8 weights
//                             are adjacent rows of the stream (t is the fastest row index of all four blocks), so a lane
//                             reads its 8 weights once and stores both; the whole stream exactly once.  Every wavefront
//                             first combines the kMaxBlocks slots of its matrix (one per lane, a butterfly of maxima)
//                             into s = clamp(floor(log2(64 / max(amax, 1e-30))), -40, 40) -- the quotient and the
//                             logarithm in float64 for fc1, float32 for the other three -- then centres (fc1 only) and
//                             scales in float64, rounds to float32 and splits into hi = half(ws), lo = half(ws -
//                             float(hi)).  Columns that hold nothing (actions beyond n_actions, inputs beyond in_dims)
//                             are stored as zeros.  Wavefront 0 of workgroup 0 writes scales[4] = 2^-s.
//
// W1 and Wav rows are in_dims and n_actions floats wide: read float by float.  W2 and W3 rows are multiples of 32
// floats wide, so their fragments are two float4 wherever the matrix itself starts on 16 bytes, and eight floats
// elsewhere (a launch-wide choice).  No product feeds a sum anywhere in this file, so there is nothing for the compiler
// to contract; the pragma below says so all the same.
#include "risvec_launch.hpp"
#include "risvec_pack.hpp"

#pragma clang fp contract(off)

// How many workgroups share the maxima of W2, Wav and W3 (1 .. 64).  A build-time constant so that an A/B build can
// measure another count (tools/time_critic_refresh.py records the one that was measured against a single workgroup).
#ifndef RISVEC_CRITIC_PACK_MAX_BLOCKS
#define RISVEC_CRITIC_PACK_MAX_BLOCKS 32
#endif

namespace risvec {
namespace {

constexpr int kMaxBlocks = RISVEC_CRITIC_PACK_MAX_BLOCKS;   // workgroups that take the maxima of W2, Wav, W3; <= 64
constexpr int kMaxK1 = 129;                      // in_dims + 1 <= 129 rows of [W1^T ; b1]
constexpr int kMeanSlots = 144;                  // 16 KS <= 144 doubles
static_assert(kMaxBlocks >= 1 && kMaxBlocks <= kWave, "one slot per lane of a wavefront");

// scales / factors / maxima are kept in the order of scales[4]: fc1, fc2, action_value, fc3
enum { kFc1 = 0, kFc2 = 1, kAv = 2, kFc3 = 3 };

struct PackArgs {
    int IN, F1, F2, F3, A;
    int KS, KSA, NG, MT2, MT3;
    int n_av, n_fc1, n_fc2, n_fc3;               // fragment-row pairs of the four blocks, in stream order
    int vec;                                     // W2 and W3 both start on 16 bytes
    const float* W1; const float* b1;            // [F1, IN], [F1]
    const float* W2;                             // [F2, F1]
    const float* Wav;                            // [F2, A]
    const float* W3;                             // [F3, F2]
    uint4* ws;                                   // [rows, 64] 16-byte fragments
    float* scales;                               // [4]
    double* mean;                                // workspace: [kMeanSlots] row means of [W1^T ; b1] (rows > IN unused)
    double* amax1;                               // workspace: [1] largest |centred fc1|
    float* amax;                                 // workspace: [3][kMaxBlocks] slices of fc2, action_value, fc3 (rows kFc2 - 1 ..)
};

__global__ void __launch_bounds__(kStatBlock)
k_sarl_critic_pack_stats(PackArgs P) {
    __shared__ double s_part[kStatWaves][kMaxK1];
    __shared__ double s_mean[kMaxK1];
    __shared__ double s_red[kStatWaves];
    __shared__ float s_redf[kStatWaves];
    if (blockIdx.x > 0) {                        // block-uniform: the barriers below are met by whole workgroups
        const int b = blockIdx.x - 1;
        const float a2 = block_max(amax_slice(P.W2, (long long)P.F2 * P.F1, b, kMaxBlocks), s_redf);
        const float aa = block_max(amax_slice(P.Wav, (long long)P.F2 * P.A, b, kMaxBlocks), s_redf);
        const float a3 = block_max(amax_slice(P.W3, (long long)P.F3 * P.F2, b, kMaxBlocks), s_redf);
        if (threadIdx.x == 0) {
            P.amax[(kFc2 - 1) * kMaxBlocks + b] = a2;
            P.amax[(kAv - 1) * kMaxBlocks + b] = aa;
            P.amax[(kFc3 - 1) * kMaxBlocks + b] = a3;
        }
        return;
    }
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int IN = P.IN, F1 = P.F1;

    // row k of [W1^T ; b1] is column k of W1 (k < IN) or b1 (k = IN); this lane owns rows lane, lane + 64, lane + 128.
    // Sum of row k: wavefront w adds features w, w + 16, ... in that order, then the 16 partial sums in wavefront order.
    auto value = [&](int f, int k) { return (double)(k < IN ? P.W1[(size_t)f * IN + k] : P.b1[f]); };
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int f = wave; f < F1; f += kStatWaves)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = lane + kWave * c;
            if (k <= IN) acc[c] += value(f, k);
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int k = lane + kWave * c;
        if (k <= IN) s_part[wave][k] = acc[c];
    }
    __syncthreads();
    if ((int)threadIdx.x <= IN) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < kStatWaves; ++w) s += s_part[w][threadIdx.x];
        const double m = s / (double)F1;
        s_mean[threadIdx.x] = m;
        P.mean[threadIdx.x] = m;
    }
    __syncthreads();

    // largest magnitude of the centred fc1 operand
    double a1 = 0.0;
#pragma unroll 4
    for (int f = wave; f < F1; f += kStatWaves)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = lane + kWave * c;
            if (k <= IN) a1 = fmax(a1, fabs(value(f, k) - s_mean[k]));
        }
    a1 = block_max(a1, s_red);
    if (threadIdx.x == 0) P.amax1[0] = a1;
}

// the shift s of matrix `which` (wave-uniform), every lane of the wavefront taking part
__device__ __forceinline__ int shift_of(const PackArgs& P, int which, int lane) {
    if (which == kFc1)                           // a float64 operand: the quotient and the logarithm in float64
        return (int)fmin(fmax(floor(log2(64.0 / fmax(P.amax1[0], 1e-30))), -40.0), 40.0);
    return shift_of_slots(lane < kMaxBlocks ? P.amax[(which - 1) * kMaxBlocks + lane] : 0.0f);
}

__global__ void __launch_bounds__(kPackBlock)
k_sarl_critic_pack(PackArgs P) {
    // pr, the pair of fragment rows, is the same for the 64 lanes of a wavefront: every branch below is wave-uniform
    // but the column guards
    const int idx = blockIdx.x * kPackBlock + threadIdx.x;       // < 2^31: at most 2560 pairs of rows
    const int lane = idx & (kWave - 1), r = lane & 31, h = lane >> 5;
    int q = idx >> 6;
    const long long pr = q;
    if (q == 0) {                                                // wavefront 0 of workgroup 0: the four scales
        float u = 0.0f;
        for (int i = 0; i < 4; ++i) {
            const int s = shift_of(P, i, lane);
            if (lane == i) u = ldexpf(1.0f, -s);
        }
        if (lane < 4) P.scales[lane] = u;
    }
    float w[8];
    if (q < P.n_av) {                                            // pair ((wv KSA + s) MT2 + m): X = Wav^T, zero padded
        const double mult = ldexp(1.0, shift_of(P, kAv, lane));
        const int wv = q / (P.KSA * P.MT2), s = (q / P.MT2) % P.KSA, m = q % P.MT2;
        const int n = 32 * (wv * P.MT2 + m) + r, A = P.A;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * s + 8 * h + j;
            w[j] = k < A ? (float)((double)P.Wav[(size_t)n * A + k] * mult) : 0.0f;
        }
    } else if ((q -= P.n_av) < P.n_fc1) {                        // pair (g KS + s): the centred [W1 | b1 | 0]
        const double mult = ldexp(1.0, shift_of(P, kFc1, lane));
        const int f = 32 * (q / P.KS) + r, s = q % P.KS, IN = P.IN;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * s + 8 * h + j;
            double x = 0.0;
            if (k < IN) x = (double)P.W1[(size_t)f * IN + k] - P.mean[k];
            else if (k == IN) x = (double)P.b1[f] - P.mean[k];
            w[j] = (float)(x * mult);
        }
    } else if ((q -= P.n_fc1) < P.n_fc2) {                       // pair ((wv 2 NG + k) MT2 + m): X = W2^T
        const double mult = ldexp(1.0, shift_of(P, kFc2, lane));
        const int ks = 2 * P.NG, wv = q / (ks * P.MT2), k = (q / P.MT2) % ks, m = q % P.MT2;
        acc_order_weights(P.W2, P.F1, 32 * (wv * P.MT2 + m) + r, 16 * k + 4 * h, P.vec != 0, mult, w);
    } else if ((q -= P.n_fc2) < P.n_fc3) {                       // pair ((wv fc2 / 16 + k) MT3 + m): X = W3^T
        const double mult = ldexp(1.0, shift_of(P, kFc3, lane));
        const int ks = 8 * P.MT2, wv = q / (ks * P.MT3), k = (q / P.MT3) % ks, m = q % P.MT3;
        acc_order_weights(P.W3, P.F2, 32 * (wv * P.MT3 + m) + r, 16 * k + 4 * h, P.vec != 0, mult, w);
    } else {
        return;                                                  // the last workgroup's spare wavefronts
    }
    store_pair(P.ws, pr, lane, w);
}

}  // namespace

long long sarl_critic_pack_workspace(int IN, int F1, int F2, int F3, int A) {
    if (!sarl_critic_supported(IN, F1, F2, F3, A)) return 0;
    return (long long)(kMeanSlots + 2) * (long long)sizeof(double) + 3LL * kMaxBlocks * (long long)sizeof(float);
}

hipError_t launch_sarl_critic_pack(int IN, int F1, int F2, int F3, int A, const float* W1, const float* b1, const float* W2,
                                   const float* Wav, const float* W3, void* wstream, float* scales, void* workspace,
                                   hipStream_t st) {
    if (!sarl_critic_supported(IN, F1, F2, F3, A)) return hipErrorInvalidValue;
    const int KS = ks_of(IN + 1), KSA = ks_of(A), NG = F1 / 32, MT2 = F2 / 128, MT3 = F3 / 128;
    const CriticLayout L = critic_layout(KS, KSA, NG, MT2, MT3);     // a block's pairs: half its rows
    double* wsp = static_cast<double*>(workspace);
    const bool vec = ((reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(W3)) & 15u) == 0;
    PackArgs a{IN, F1, F2, F3, A, KS, KSA, NG, MT2, MT3,
               (int)((L.fc1 - L.av) / 2), (int)((L.fc2 - L.fc1) / 2), (int)((L.fc3 - L.fc2) / 2), (int)((L.rows - L.fc3) / 2), vec ? 1 : 0,
               W1, b1, W2, Wav, W3, static_cast<uint4*>(wstream), scales,
               wsp, wsp + kMeanSlots, reinterpret_cast<float*>(wsp + kMeanSlots + 2)};
    // the pairs of rows in all: half the rows of sarl_critic_stream_bytes()
    const long long pairs = (long long)a.n_av + a.n_fc1 + a.n_fc2 + a.n_fc3;
    if (pairs * 2048 != sarl_critic_stream_bytes(IN, F1, F2, F3, A)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sarl_critic_pack_stats, dim3(1 + kMaxBlocks), dim3(kStatBlock), 0, st, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    note_kernel("k_sarl_critic_pack");
    hipLaunchKernelGGL(k_sarl_critic_pack, dim3((unsigned)((pairs * kWave + kPackBlock - 1) / kPackBlock)), dim3(kPackBlock), 0,
                       st, a);
    return hipGetLastError();
}

}  // namespace risvec
