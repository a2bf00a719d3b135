// The weight streams of k_marl_critic.hip, built on the device from the float32 weights of n_nets in {1, 2} nets in two
// launches: what pack_marl_critic_weights (ris_vec_marl_amd/marl_critic.py) computes with library kernels once per net,
// element for element.
//
//   k_marl_critic_pack_stats  kMaxBlocks x n_nets workgroups that never talk to each other.  Workgroup (b, c) takes slice b
//                             of W1, of W2 and of W3 of net c and leaves the largest magnitude of each in slot
//                             [c][matrix][b] of the workspace.  A maximum does not depend on the order it is taken in, a
//                             slot has one writer, every slot is written: no atomics, no counters, nothing to initialise.
//   k_marl_critic_pack        one lane per PAIR of 16-byte fragments: the hi and the lo fragment of the same 8 weights
//                             are adjacent rows of the stream (t is the fastest row index of all three blocks), so a lane
//                             reads its 8 weights once and stores both; every stream exactly once.  blockIdx.y is the
//                             net.  Every wavefront first combines the kMaxBlocks slots of its net's matrix (one per
//                             lane, a butterfly of maxima) into s = clamp(floor(log2f(64 / max(amax, 1e-30))), -40, 40)
//                             -- the quotient and the logarithm in float32 for all three: this net's fc1 operand is the
//                             float32 weight itself, not a centred float64 one -- then scales in float64, rounds to
//                             float32 and splits into hi = half(ws), lo = half(ws - float(hi)).  fc1 columns beyond
//                             state_dims + action_dims are stored as zeros.  Wavefront 0 of each net writes that net's
//                             scales[3] = 2^-s.
//
// W1 rows are state_dims + action_dims floats wide: read float by float.  W2 and W3 rows are multiples of 32 floats wide,
// so their fragments are two float4 wherever every such matrix of the call starts on 16 bytes, and eight floats
// elsewhere (a launch-wide choice).  No product feeds a sum anywhere in this file, so there is nothing for the compiler
// to contract; the pragma below says so all the same.
#include "risvec_launch.hpp"
#include "risvec_pack.hpp"

#pragma clang fp contract(off)

// How many workgroups per net share the maxima of W1, W2 and W3 (1 .. 64).  A build-time constant so that an A/B build
// can measure another count (tools/time_marl_critic_refresh.py records the one that was measured against a single
// workgroup).
#ifndef RISVEC_MARL_CRITIC_PACK_MAX_BLOCKS
#define RISVEC_MARL_CRITIC_PACK_MAX_BLOCKS 32
#endif

namespace risvec {
namespace {

constexpr int kMaxBlocks = RISVEC_MARL_CRITIC_PACK_MAX_BLOCKS;   // workgroups per net that take the maxima; <= 64
constexpr int kMaxNets = 2;
static_assert(kMaxBlocks >= 1 && kMaxBlocks <= kWave, "one slot per lane of a wavefront");

// scales / maxima are kept in the order of scales[3]: fc1, fc2, fc3
enum { kFc1 = 0, kFc2 = 1, kFc3 = 2 };

struct PackNet {
    const float* W1;                             // [F1, IN]
    const float* W2;                             // [F2, F1]
    const float* W3;                             // [F3, F2]
    uint4* ws;                                   // [rows, 64] 16-byte fragments
    float* scales;                               // [3]
};

struct PackArgs {
    int IN, F1, F2, F3;
    int KS, NG, MT2, MT3;
    int n_fc1, n_fc2, n_fc3;                     // fragment-row pairs of the three blocks, in stream order
    int vec;                                     // W2 and W3 of every net start on 16 bytes
    PackNet net[kMaxNets];
    float* amax;                                 // workspace: [n_nets][3][kMaxBlocks] slices of fc1, fc2, fc3
};

// net c of the call (c is uniform over the workgroup): a select per field, never an indexed copy of the argument block
__device__ __forceinline__ PackNet net_of(const PackArgs& P, int c) {
    return PackNet{c ? P.net[1].W1 : P.net[0].W1, c ? P.net[1].W2 : P.net[0].W2, c ? P.net[1].W3 : P.net[0].W3,
                   c ? P.net[1].ws : P.net[0].ws, c ? P.net[1].scales : P.net[0].scales};
}

// the largest of v over the workgroup (order-independent); red: kStatWaves slots of LDS.  The float32 form with fmaxf:
// this file's own, chosen over the template of risvec_pack.hpp (a compare and a select), which compiles differently
__device__ __forceinline__ float block_max(float v, float* red) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < kStatWaves; ++i) r = fmaxf(r, red[i]);
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kStatBlock)
k_marl_critic_pack_stats(PackArgs P) {
    __shared__ float s_red[kStatWaves];
    const int b = blockIdx.x, c = blockIdx.y;
    const PackNet N = net_of(P, c);
    const float a1 = block_max(amax_slice(N.W1, (long long)P.F1 * P.IN, b, kMaxBlocks), s_red);
    const float a2 = block_max(amax_slice(N.W2, (long long)P.F2 * P.F1, b, kMaxBlocks), s_red);
    const float a3 = block_max(amax_slice(N.W3, (long long)P.F3 * P.F2, b, kMaxBlocks), s_red);
    if (threadIdx.x == 0) {
        float* slot = P.amax + (size_t)c * 3 * kMaxBlocks + b;
        slot[kFc1 * kMaxBlocks] = a1;
        slot[kFc2 * kMaxBlocks] = a2;
        slot[kFc3 * kMaxBlocks] = a3;
    }
}

// the shift s of matrix `which` of net c (wave-uniform), every lane of the wavefront taking part
__device__ __forceinline__ int shift_of(const PackArgs& P, int c, int which, int lane) {
    return shift_of_slots(lane < kMaxBlocks ? P.amax[((size_t)c * 3 + which) * kMaxBlocks + lane] : 0.0f);
}

__global__ void __launch_bounds__(kPackBlock)
k_marl_critic_pack(PackArgs P) {
    // pr, the pair of fragment rows, is the same for the 64 lanes of a wavefront: every branch below is wave-uniform
    // but the column guard of fc1
    const int idx = blockIdx.x * kPackBlock + threadIdx.x;       // < 2^31: at most 2560 pairs of rows per net (2304 at 512 inputs)
    const int lane = idx & (kWave - 1), r = lane & 31, h = lane >> 5;
    const int c = blockIdx.y;
    int q = idx >> 6;
    const long long pr = q;
    if (q >= P.n_fc1 + P.n_fc2 + P.n_fc3) return;                // the last workgroup's spare wavefronts
    const PackNet N = net_of(P, c);
    if (q == 0) {                                                // wavefront 0 of this net: its three scales
        float u = 0.0f;
        for (int i = 0; i < 3; ++i) {
            const int s = shift_of(P, c, i, lane);
            if (lane == i) u = ldexpf(1.0f, -s);
        }
        if (lane < 3) N.scales[lane] = u;
    }
    float w[8];
    if (q < P.n_fc1) {                                           // pair (g KS + s): [W1 | 0]
        const double mult = ldexp(1.0, shift_of(P, c, kFc1, lane));
        const int f = 32 * (q / P.KS) + r, s = q % P.KS, IN = P.IN;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * s + 8 * h + j;
            w[j] = k < IN ? (float)((double)N.W1[(size_t)f * IN + k] * mult) : 0.0f;
        }
    } else if ((q -= P.n_fc1) < P.n_fc2) {                       // pair ((wv 2 NG + k) MT2 + m): X = W2^T
        const double mult = ldexp(1.0, shift_of(P, c, kFc2, lane));
        const int ks = 2 * P.NG, wv = q / (ks * P.MT2), k = (q / P.MT2) % ks, m = q % P.MT2;
        acc_order_weights(N.W2, P.F1, 32 * (wv * P.MT2 + m) + r, 16 * k + 4 * h, P.vec != 0, mult, w);
    } else {                                                     // pair ((wv fc2 / 16 + k) MT3 + m): X = W3^T
        q -= P.n_fc2;
        const double mult = ldexp(1.0, shift_of(P, c, kFc3, lane));
        const int ks = 8 * P.MT2, wv = q / (ks * P.MT3), k = (q / P.MT3) % ks, m = q % P.MT3;
        acc_order_weights(N.W3, P.F2, 32 * (wv * P.MT3 + m) + r, 16 * k + 4 * h, P.vec != 0, mult, w);
    }
    store_pair(N.ws, pr, lane, w);
}

long long workspace_bytes(int n_nets) {
    const long long bytes = (long long)n_nets * 3 * kMaxBlocks * (long long)sizeof(float);
    return (bytes + 15) / 16 * 16;
}

// The two launches for a shape one of the two rules covers; stream_bytes: what that rule's *_stream_bytes() states
hipError_t launch_pack(int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticPackNet* nets, void* workspace,
                       long long stream_bytes, hipStream_t st) {
    const int IN = S + A, KS = ks_of(IN), NG = F1 / 32, MT2 = F2 / 128, MT3 = F3 / 128;
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);              // a block's pairs: half its rows
    PackArgs a{};
    a.IN = IN; a.F1 = F1; a.F2 = F2; a.F3 = F3; a.KS = KS; a.NG = NG; a.MT2 = MT2; a.MT3 = MT3;
    a.n_fc1 = (int)((L.fc2 - L.fc1) / 2); a.n_fc2 = (int)((L.fc3 - L.fc2) / 2); a.n_fc3 = (int)((L.rows - L.fc3) / 2);
    // the pairs of rows in all: half the rows of the stream
    const long long pairs = (long long)a.n_fc1 + a.n_fc2 + a.n_fc3;
    if (pairs * 2048 != stream_bytes) return hipErrorInvalidValue;
    uintptr_t align = 0;
    for (int i = 0; i < kMaxNets; ++i) {
        const RisVecMarlCriticPackNet& n = nets[i < n_nets ? i : 0];  // the unused slot of a single net repeats net 1
        a.net[i] = PackNet{n.W1, n.W2, n.W3, static_cast<uint4*>(n.wstream), n.scales};
        align |= reinterpret_cast<uintptr_t>(n.W2) | reinterpret_cast<uintptr_t>(n.W3);
    }
    a.vec = (align & 15u) == 0 ? 1 : 0;
    a.amax = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_marl_critic_pack_stats, dim3(kMaxBlocks, n_nets), dim3(kStatBlock), 0, st, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    note_kernel("k_marl_critic_pack x%d", n_nets);
    hipLaunchKernelGGL(k_marl_critic_pack, dim3((unsigned)((pairs * kWave + kPackBlock - 1) / kPackBlock), n_nets),
                       dim3(kPackBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace

long long marl_critic_pack_workspace(int S, int A, int F1, int F2, int F3, int n_nets) {
    if (!marl_critic_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > kMaxNets) return 0;
    return workspace_bytes(n_nets);
}

long long marl_critic_wide_pack_workspace(int S, int A, int F1, int F2, int F3, int n_nets) {
    if (!marl_critic_wide_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > kMaxNets) return 0;
    return workspace_bytes(n_nets);
}

hipError_t launch_marl_critic_pack(int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticPackNet* nets,
                                   void* workspace, hipStream_t st) {
    if (!marl_critic_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > kMaxNets) return hipErrorInvalidValue;
    return launch_pack(S, A, F1, F2, F3, n_nets, nets, workspace, marl_critic_stream_bytes(S, A, F1, F2, F3), st);
}

hipError_t launch_marl_critic_wide_pack(int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticPackNet* nets,
                                        void* workspace, hipStream_t st) {
    if (!marl_critic_wide_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > kMaxNets) return hipErrorInvalidValue;
    return launch_pack(S, A, F1, F2, F3, n_nets, nets, workspace, marl_critic_wide_stream_bytes(S, A, F1, F2, F3), st);
}

}  // namespace risvec
