// The weight stream of k_sarl_actor.hip, built on the device from the float32 weights in two launches: what
// pack_actor_weights (ris_vec_marl_amd/actor.py) computes with library kernels, element for element.
//
//   k_sarl_actor_pack_stats   ONE workgroup.  The float64 mean over the fc1 features of every row of [W1^T ; b1], the
//                             largest magnitude of the centred fc1 operand, of W2 and of Wmu, and from those the three
//                             shifts s = clamp(floor(log2(64 / max(amax, 1e-30))), -40, 40): scales[i] = 2^-s as float32,
//                             the workspace keeps the means and 2^s as float64.  One workgroup, so that every sum runs in
//                             one fixed order and nothing is handed from one workgroup to another inside the launch: no
//                             atomics, no counters, nothing to initialise, the same bits on every run.
//   k_sarl_actor_pack         one lane per 16-byte fragment (8 halfs) of the stream, the whole stream exactly once.  A
//                             lane works out from (item, row, lane) what its fragment holds -- the inverse of the
//                             permutations in the header of k_sarl_actor.hip -- reads the 8 weights, centres (fc1 only)
//                             and scales them in float64, rounds to float32, splits into hi = half(ws) and
//                             lo = half(ws - float(hi)) and stores the half its row asks for.  Rows and columns that
//                             hold nothing are stored as zeros: the buffer is reused from call to call.
//
// The pass-1 and the pass-2 copy of an fc1 group go through the same statements (fc1_fragment) on the same inputs, so
// they are the same bits, which the forward kernel relies on.  No product feeds a sum anywhere in this file, so there
// is nothing for the compiler to contract; the pragma below says so all the same.
#include "risvec_launch.hpp"
#include "risvec_pack.hpp"

#pragma clang fp contract(off)

namespace risvec {
namespace {

constexpr int kMaxK1 = 129;                      // in_dims + 1 <= 129 rows of [W1^T ; b1]

struct PackArgs {
    int IN, F1, F2, A;
    int KS, MT, HT, NG, R, T1, items;            // the geometry of sarl_actor_geom
    const float* W1; const float* b1;            // [F1, IN], [F1]
    const float* ln1w; const float* ln1b;        // [F1]
    const float* W2;                             // [F2, F1]
    const float* Wmu;                            // [A, F2]
    uint4* ws;                                   // [items, R, 64] 16-byte fragments
    float* scales;                               // [3]
    double* mean;                                // workspace: [16 KS] row means of [W1^T ; b1] (rows > IN unused)
    double* mult;                                // workspace: [3] 2^s of fc1, fc2, mu
};

// largest |x| over n4 float4 of p, for this thread's share
__device__ __forceinline__ float amax_f4(const float4* p, int n4) {
    float m = 0.0f;
#pragma unroll 8
    for (int i = threadIdx.x; i < n4; i += kStatBlock) m = max4(m, p[i]);
    return m;
}

__global__ void __launch_bounds__(kStatBlock)
k_sarl_actor_pack_stats(PackArgs P) {
    __shared__ double s_part[kStatWaves][kMaxK1];
    __shared__ double s_mean[kMaxK1];
    __shared__ double s_red[kStatWaves];
    __shared__ float s_redf[kStatWaves];
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
    const float a2 = block_max(amax_f4(reinterpret_cast<const float4*>(P.W2), P.F2 * (F1 / 4)), s_redf);
    const float ah = block_max(amax_f4(reinterpret_cast<const float4*>(P.Wmu), P.A * (P.F2 / 4)), s_redf);

    if (threadIdx.x == 0) {
        // fc1 is a float64 operand, fc2 and mu are float32 ones: the quotient and the logarithm in the operand's precision
        const double s1 = fmin(fmax(floor(log2(64.0 / fmax(a1, 1e-30))), -40.0), 40.0);
        const float s2 = fminf(fmaxf(floorf(log2f(64.0f / fmaxf(a2, 1e-30f))), -40.0f), 40.0f);
        const float sh = fminf(fmaxf(floorf(log2f(64.0f / fmaxf(ah, 1e-30f))), -40.0f), 40.0f);
        const int s[3] = {(int)s1, (int)s2, (int)sh};
        for (int i = 0; i < 3; ++i) {
            P.mult[i] = ldexp(1.0, s[i]);
            P.scales[i] = ldexpf(1.0f, -s[i]);
        }
    }
}

// 8 scaled weights -> the hi (t = 0) or lo (t = 1) halves, as one 16-byte fragment
__device__ __forceinline__ uint4 split_fragment(const float (&w)[8], int t) {
    half8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 hi = (_Float16)w[j];
        out[j] = t == 0 ? hi : (_Float16)(w[j] - (float)hi);
    }
    return __builtin_bit_cast(uint4, out);
}

// fragment (k-step s, t) of fc1 group grp: element j = S_t[32 grp + r][16 s + 8 h + j] of the centred [W1 | b1 | 0]
__device__ __forceinline__ uint4 fc1_fragment(const PackArgs& P, int grp, int s, int t, int r, int h) {
    const int f = 32 * grp + r, IN = P.IN;
    const double mult = P.mult[0];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * s + 8 * h + j;
        double x = 0.0;
        if (k < IN) x = (double)P.W1[(size_t)f * IN + k] - P.mean[k];
        else if (k == IN) x = (double)P.b1[f] - P.mean[k];
        w[j] = (float)(x * mult);
    }
    return split_fragment(w, t);
}

// A fragment whose k index runs over an accumulator tile's rows: element j = S_t[f0 + 8 (j >> 2) + (j & 3)][n], where
// X[f][n] = W[n * ld + f] (a Linear weight [out, in] read as [in, out]); f0 a multiple of 4, so two float4 per lane
__device__ __forceinline__ uint4 acc_order_fragment(const float* W, int ld, int n, int f0, double mult, int t) {
    const float4 lo4 = *reinterpret_cast<const float4*>(W + (size_t)n * ld + f0);
    const float4 hi4 = *reinterpret_cast<const float4*>(W + (size_t)n * ld + f0 + 8);
    const float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (float)((double)v[j] * mult);
    return split_fragment(w, t);
}

__global__ void __launch_bounds__(kPackBlock)
k_sarl_actor_pack(PackArgs P) {
    // (item, row) is the same for the 64 lanes of a wavefront: every branch below is wave-uniform but the column guards
    const int idx = blockIdx.x * kPackBlock + threadIdx.x;       // < items R 64 (the grid is exact), < 2^31
    const int lane = idx & (kWave - 1), r = lane & 31, h = lane >> 5;
    const int row = (idx >> 6) % P.R, item = (idx >> 6) / P.R;
    const int KS = P.KS, MT = P.MT, HT = P.HT, NG = P.NG;
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if (item < P.T1) {                                           // pass 1: P1 groups of 2 KS rows, the tail zero
        const int at = row / (2 * KS), q = row % (2 * KS), grp = item * (P.R / (2 * KS)) + at;
        if (at < P.R / (2 * KS) && grp < NG) out = fc1_fragment(P, grp, q >> 1, q & 1, r, h);
    } else if (item < P.T1 + NG) {                               // pass 2: fc1 again | LayerNorm-1 | fc2 | zero rows
        const int grp = item - P.T1, q = row - (2 * KS + 1);
        if (row < 2 * KS) {
            out = fc1_fragment(P, grp, row >> 1, row & 1, r, h);
        } else if (row == 2 * KS) {                              // 256 floats: [32 weights | 32 biases | zeros]
            if (lane < 16) {
                const float* src = (lane < 8 ? P.ln1w : P.ln1b) + 32 * grp + 4 * (lane & 7);
                out = __builtin_bit_cast(uint4, *reinterpret_cast<const float4*>(src));
            }
        } else if (q < 4 * MT) {                                 // row = (2 u + t) MT + m
            const int u = q / (2 * MT), t = (q / MT) & 1, m = q % MT;
            out = acc_order_fragment(P.W2, P.F1, 32 * m + r, 32 * grp + 16 * u + 4 * h, P.mult[1], t);
        }
    } else {                                                     // head: HS k-steps of 2 HT rows, the tail zero
        const int HS = P.R / (2 * HT), at = row / (2 * HT), q = row % (2 * HT);
        const int st = (item - P.T1 - NG) * HS + at, a = 32 * (q >> 1) + r;
        if (at < HS && st < 2 * MT && a < P.A)                   // k-step st = 2 m + u: rows 16 st + ... of [F2, 32 HT]
            out = acc_order_fragment(P.Wmu, P.F2, a, 16 * st + 4 * h, P.mult[2], q & 1);
    }
    P.ws[idx] = out;
}

}  // namespace

long long sarl_actor_pack_workspace(int IN, int F1, int F2, int A) {
    const SarlActorGeom g = sarl_actor_geom(IN, F1, F2, A);
    return g.items == 0 ? 0 : (long long)(16 * g.ks + 4) * (long long)sizeof(double);
}

hipError_t launch_sarl_actor_pack(int IN, int F1, int F2, int A, const float* W1, const float* b1, const float* ln1w,
                                  const float* ln1b, const float* W2, const float* Wmu, void* wstream, float* scales,
                                  void* workspace, hipStream_t st) {
    const SarlActorGeom g = sarl_actor_geom(IN, F1, F2, A);
    if (g.items == 0) return hipErrorInvalidValue;
    double* wsp = static_cast<double*>(workspace);
    PackArgs a{IN, F1, F2, A, g.ks, g.mt, g.ht, g.ng, g.rows, g.t1, g.items, W1, b1, ln1w, ln1b, W2, Wmu,
               static_cast<uint4*>(wstream), scales, wsp, wsp + 16 * g.ks};
    hipLaunchKernelGGL(k_sarl_actor_pack_stats, dim3(1), dim3(kStatBlock), 0, st, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    // rows is a multiple of 4, so the stream is a whole number of 256-lane workgroups
    note_kernel("k_sarl_actor_pack");
    hipLaunchKernelGGL(k_sarl_actor_pack, dim3((unsigned)(g.items * g.rows * kWave / kPackBlock)), dim3(kPackBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace risvec
