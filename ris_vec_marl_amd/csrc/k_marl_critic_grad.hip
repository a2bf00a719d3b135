// The critic loss of the multi-agent (SAC) learner and its gradients (Global_SAC_Critic.global_learn,
// Simulation-MARL-BCD/global_sac_critic.py:355-363) without an autograd graph, in TWO launches, for n rows and n_nets in
// {1, 2} CriticNetworks (networks.py:38-49) of one shape, per net c:
//     x = [state | action]   h1 = relu(W1 x + b1)   h2 = relu(W2 h1 + b2)   h3 = relu(W3 h2 + b3)   q = wq . h3 + bq
//     e = (2 / n) (q - y)                       y: the TD target, a constant, read in place
//     loss = sum_c (1 / n) sum_b (q_c[b] - y[b])^2
//     d3 = (e wq) * [h3 > 0]    d2 = (W3^T d3) * [h2 > 0]    d1 = (W2^T d2) * [h1 > 0]
//     d wq = sum_b e h3    d bq = sum_b e    d Wl = dl^T a(l-1)  (a0 = x)    d bl = sum_b dl
// The gradients are overwritten, never accumulated.  Orientation, precision and register order are those of
// risvec_mfma.hpp (read its header); the forward is the walk of risvec_critic_walk.hpp on the packed weight stream.
//
// 1  k_marl_critic_grad_rows<MT2, MT3>: grid (32-row tiles, nets), four wavefronts per tile.  The forward is the
//    shared walk (marl_stage_input, critic_fc1_walk, critic_fc2) with callbacks that also send every activation tile to the
//    workspace as it is produced; only the fc3 block is this kernel's own, because d3 is formed in its registers.  Then, in
//    the same workgroup:
//      d3 is formed in registers (the fc3 tiles are still there) and goes to LDS as B fragments, exactly as put_tile
//         leaves a layer's output for the next MFMA: registers 8u .. 8u+7 = k-step 2 tile + u;
//      d2 = W3^T d3: wavefront w owns the fc2 tiles it owned in the forward, so the lane that wrote h2[f][row] applies its
//         mask; the result goes to LDS the same way;
//      d1 = W2^T d2: wavefront w owns fc1 groups w, w + 4, .., as in the forward; the result goes out.
//    The transposed products read the FLOAT32 WEIGHTS IN PLACE: the A operand of lane (i, h) at k-step s is
//    W[16 s + 8 (j >> 2) + 4 h + (j & 3)][i0 + i], j = 0..7 -- the permuted k order in which put_tile left the deltas --
//    eight dword loads, each coalesced over 32 lanes, multiplied by the exact power of two that the forward stream's
//    `scales` records for the matrix (its largest entry lands in [64, 128)) and split on the fly.
//    The deltas are of order (q - y) / n and smaller, below float16's normal range at a small TD error: before the split a
//    tile's d3 / d2 is multiplied by the exact power of two that brings the tile's largest entry into [64, 128), and the
//    accumulator is multiplied back.
//    LDS: s_in as in the forward; s_h holds h1's fragments, then h2's in [0, fc2 / 16) and d3's in [fc2 / 16, fc2 / 16 +
//    fc3 / 16), then d2's in [0, fc2 / 16) once h2 is dead: max(2 NG, (fc2 + fc3) / 16) k-steps, 145 KiB at most.
//    The ReLU masks of h2 and h1 are read back from the workspace by the lane that wrote them.
//    Workspace, float32, npad = n rounded up to 32: x [XF][npad] (XF = S + A rounded up to 32, zero beyond S + A; written
//    by the workgroups of net 0), and per net h1 h2 h3 d1 d2 d3 FEATURE-MAJOR [F][npad] -- a lane's 16 features of a row
//    are 16 stores of 128 contiguous bytes per half-wave -- then e [npad], q - y [npad], and the tiles' largest |dl|
//    [3][tiles].  Rows >= n of the last tile carry e = 0; no state, action or target row >= n is read (such a row walks
//    row 0's input, as in the forward).  Every workspace element that launch 2 reads is written by every call.
//
// 2  k_marl_critic_grad_weights: one wavefront per 32 x 32 tile of every d Wl of every net, mfma3 over npad / 16 k-steps of
//    the batch with A = dl (rows = output features) and B = a(l-1) (columns = input features), both read as two float4 per
//    lane and k-step.  dl is multiplied by one exact power of two per layer and net -- from the largest of the tiles'
//    maxima, into [64, 128) -- and the accumulator multiplied back; the activations are split unscaled.  The tiles of
//    column block 0 also sum d bl; fc3 / 8 more wavefronts sum d wq (eight lanes per feature), and one sums d bq of every net
//    and the loss.  Those sums run in float64 in a fixed order and are rounded once.  One wavefront owns each output
//    element: no atomics, the same bits on every call.
//
// Every barrier sits under wave-uniform control flow.  No global address depends on loaded data.
#include "risvec_critic_grad.hpp"
#include "risvec_critic_walk.hpp"
#include "risvec_launch.hpp"
#include "risvec_mfma.hpp"

namespace risvec {
namespace {

struct GradNetPtrs {
    MarlNetPtrs fwd;
    const float* W2;               // [F2, F1]
    const float* W3;               // [F3, F2]
    float* h1; float* h2; float* h3;   // [F][npad]
    float* d1; float* d2; float* d3;   // [F][npad]
    float* e;                      // [npad]
    float* diff;                   // [npad] q - y
    float* tmax;                   // [3][tiles]: layer 1, 2, 3
    float* q;                      // [n_rows]
};

struct GradRowArgs {
    int n_rows, S, NA, KS, NG, F1, F2, F3, XF;
    long long npad;
    const float* state;
    const float* action;
    const float* target;
    float* x;                      // [XF][npad]
    GradNetPtrs net[2];
};

// a C/D tile -> feature-major memory: features f0 + (q & 3) + 8 (q >> 2) + 4 h of column `col`
__device__ __forceinline__ void store_tile(float* ws, int f0, const f32x16_t& y, long long npad, long long col, int h) {
#pragma unroll
    for (int q = 0; q < 16; ++q) ws[(size_t)(f0 + (q & 3) + 8 * (q >> 2) + 4 * h) * npad + col] = y[q];
}

__device__ __forceinline__ f32x16_t load_tile(const float* ws, int f0, long long npad, long long col, int h) {
    f32x16_t y;
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] = ws[(size_t)(f0 + (q & 3) + 8 * (q >> 2) + 4 * h) * npad + col];
    return y;
}

template <int MT2, int MT3>
__global__ void __launch_bounds__(kMcBlock)
k_marl_critic_grad_rows(GradRowArgs A) {
    constexpr int K3 = 8 * MT2;                               // fc3 k-steps = fc2 / 16
    constexpr int K4 = 8 * MT3;                               // k-steps of d3 = fc3 / 16
    extern __shared__ uint4 s_mem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int KS = A.KS, NG = A.NG;
    const int netc = blockIdx.y;                              // uniform over the workgroup
    const GradNetPtrs& G = A.net[netc];
    const MarlNetPtrs& P = G.fwd;
    uint4* s_in = s_mem;                                      // [KS][2][64]
    uint4* s_h = s_mem + KS * 2 * kWave;                      // [max(2 NG, K3 + K4)][2][64]
    const int hsteps = max(2 * NG, K3 + K4);
    float* s_red = reinterpret_cast<float*>(s_h + hsteps * 2 * kWave);   // [kRedSlots][4][32]
    float* s_max = s_red + kCriticWaves * 32;                     // slot 1 of s_red: [3][4] maxima
    uint4* s_d3 = s_h + K3 * 2 * kWave;                       // the d3 fragments, beside h2's
    const MarlLayout L = marl_layout(KS, NG, MT2, MT3);
    const long long e0 = (long long)blockIdx.x * 32, npad = A.npad, col = e0 + r;
    const int ntiles = (int)(npad / 32);

    // ---- the input as split B fragments, and feature-major to the workspace
    marl_stage_input(A.state, A.action, A.S, A.NA, A.n_rows, s_in, e0, 0, KS, tid);
    if (netc == 0) {
        const int S = A.S, W = A.S + A.NA;
        for (int idx = tid; idx < A.XF * 32; idx += kMcBlock) {
            const int k = idx >> 5, rr = idx & 31;
            const long long row = e0 + rr < A.n_rows ? e0 + rr : 0;
            A.x[(size_t)k * npad + e0 + rr] = k < S ? A.state[row * S + k] : (k < W ? A.action[row * A.NA + (k - S)] : 0.0f);
        }
    }
    __syncthreads();

    const float u1 = P.scales[0], u2 = P.scales[1], u3 = P.scales[2];
    // ---- fc1: bias, ReLU, the split fragments to LDS and the tile to the workspace
    critic_fc1_walk(P.ws + L.fc1 * kWave, s_in, KS, NG, wave, lane, [&](int g, const f32x16_t& d) {
        const f32x16_t y = bias_relu(d, u1, tile_of(P.b1, 32 * g, h));
        put_tile(s_h, g, y, lane);
        store_tile(G.h1, 32 * g, y, npad, col, h);
    });
    __syncthreads();

    // ---- fc2, each output tile also to the workspace
    critic_fc2<MT2>(P, s_h, L, NG, wave, lane, u2, [&](int t, const f32x16_t& y) { store_tile(G.h2, 32 * t, y, npad, col, h); });

    // ---- fc3 + ReLU, the q dot product, and d3 = e wq [h3 > 0] in the registers of the fc3 tiles: critic_fc3_q with the
    // store of h3 and the mask of d3 in its loop, so it stays this kernel's own
    f32x16_t d3[MT3];
    {
        f32x16_t a3[MT3];
#pragma unroll
        for (int m = 0; m < MT3; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) a3[m][q] = 0.0f;
        gemm_tiles<MT3>(a3, P.ws + (L.fc3 + (long long)wave * K3 * MT3 * 2) * kWave, s_h, K3, lane);
        f32x16_t qs;
#pragma unroll
        for (int m = 0; m < MT3; ++m) {
            const int f0 = 32 * (wave * MT3 + m);
            const f32x16_t y = bias_relu(a3[m], u3, tile_of(P.b3, f0, h));
            store_tile(G.h3, f0, y, npad, col, h);
            const f32x16_t qw = tile_of(P.qw, f0, h);
            const f32x16_t p = y * qw;
            qs = m == 0 ? p : qs + p;
#pragma unroll
            for (int q = 0; q < 16; ++q) d3[m][q] = y[q] > 0.0f ? qw[q] : 0.0f;      // e is applied below
        }
        float qp = sum16(qs);
        qp += __shfl_xor(qp, 32, kWave);
        if (h == 0) s_red[wave * 32 + r] = qp;
    }
    __syncthreads();                                          // every wavefront is past its fc3 MFMAs: h2's fragments are dead

    const bool live = col < A.n_rows;
    const float qv = marl_red(s_red, 0, r) + P.qb[0];         // every lane of every wavefront: the same sum in the same order
    const float diff = live ? qv - A.target[col] : 0.0f;
    const float e = diff * (2.0f / (float)A.n_rows);
    if (wave == 0 && h == 0) {
        if (live) G.q[col] = qv;
        G.e[col] = e;
        G.diff[col] = diff;
    }
    float mx = 0.0f;
#pragma unroll
    for (int m = 0; m < MT3; ++m) {
        d3[m] = d3[m] * e;
        store_tile(G.d3, 32 * (wave * MT3 + m), d3[m], npad, col, h);
        mx = absmax16(d3[m], mx);
    }
    mx = wave_max(mx);
    if (lane == 0) s_max[8 + wave] = mx;
    __syncthreads();
    const float m3 = fmaxf(fmaxf(s_max[8], s_max[9]), fmaxf(s_max[10], s_max[11]));
    const int s3 = grad_scale_exp(m3);
    if (tid == 0) G.tmax[2 * ntiles + blockIdx.x] = m3;
    {
        const float up = ldexpf(1.0f, s3);
#pragma unroll
        for (int m = 0; m < MT3; ++m) put_tile(s_d3, wave * MT3 + m, d3[m] * up, lane);
    }
    __syncthreads();

    // ---- d2 = (W3^T d3) [h2 > 0]: the fc2 tiles this wavefront owned in the forward
    {
        f32x16_t acc[MT2];
#pragma unroll
        for (int m = 0; m < MT2; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
        gemm_tiles_t<MT2>(acc, G.W3, A.F2, 32 * wave * MT2, 1.0f / u3, s_d3, K4, lane);
        const float back = u3 * ldexpf(1.0f, -s3);
        mx = 0.0f;
#pragma unroll
        for (int m = 0; m < MT2; ++m) {
            const int t = wave * MT2 + m;
            const f32x16_t hh = load_tile(G.h2, 32 * t, npad, col, h);        // this lane's own stores
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][q] = hh[q] > 0.0f ? acc[m][q] * back : 0.0f;
            store_tile(G.d2, 32 * t, acc[m], npad, col, h);
            mx = absmax16(acc[m], mx);
        }
        mx = wave_max(mx);
        if (lane == 0) s_max[4 + wave] = mx;
        __syncthreads();
        const float m2 = fmaxf(fmaxf(s_max[4], s_max[5]), fmaxf(s_max[6], s_max[7]));
        const int s2 = grad_scale_exp(m2);
        if (tid == 0) G.tmax[ntiles + blockIdx.x] = m2;
        const float up = ldexpf(1.0f, s2);
#pragma unroll
        for (int m = 0; m < MT2; ++m) put_tile(s_h, wave * MT2 + m, acc[m] * up, lane);
        __syncthreads();

        // ---- d1 = (W2^T d2) [h1 > 0]: fc1 groups wave, wave + 4, ..
        const float back1 = u2 * ldexpf(1.0f, -s2);
        mx = 0.0f;
        for (int g = wave; g < NG; g += kCriticWaves) {
            f32x16_t a1[1];
#pragma unroll
            for (int q = 0; q < 16; ++q) a1[0][q] = 0.0f;
            gemm_tiles_t<1>(a1, G.W2, A.F1, 32 * g, 1.0f / u2, s_h, K3, lane);
            const f32x16_t hh = load_tile(G.h1, 32 * g, npad, col, h);        // this lane's own stores
#pragma unroll
            for (int q = 0; q < 16; ++q) a1[0][q] = hh[q] > 0.0f ? a1[0][q] * back1 : 0.0f;
            store_tile(G.d1, 32 * g, a1[0], npad, col, h);
            mx = absmax16(a1[0], mx);
        }
        mx = wave_max(mx);
        if (lane == 0) s_max[wave] = mx;
        __syncthreads();
        if (tid == 0) G.tmax[blockIdx.x] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct GradWNet {
    const float* h1; const float* h2; const float* h3;
    const float* d1; const float* d2; const float* d3;
    const float* e; const float* diff; const float* tmax;
    float* dW1; float* db1; float* dW2; float* db2; float* dW3; float* db3; float* dqw; float* dqb;
};

struct GradWArgs {
    int n_rows, n_nets, IN, F1, F2, F3, ntiles;
    int c1, t1, t2, t3, tq, per_net;                          // fc1 column tiles; items per kind and per net
    long long npad;
    const float* x;
    GradWNet net[2];
    float* loss;
};

constexpr int kGwBlock = 256;        // four independent wavefronts, one item each
constexpr int kGwFeat = 8;           // features of d wq per wavefront

// One 32 x 32 tile of d W = dl^T a: rows [i0, i0 + 32) of dl [F][npad], columns [c0, c0 + 32) of a [F'][npad], and with db
// the bias sums of those rows
__device__ __forceinline__ void grad_w_tile(const float* dl, const float* a, const float* tmax, int ntiles, long long npad, int i0, int c0,
                                            float* dW, int ld, float* db, int lane) {
    const int i = lane & 31, h = lane >> 5;
    float amax = 0.0f;
    for (int t = lane; t < ntiles; t += kWave) amax = fmaxf(amax, tmax[t]);
    const int sx = grad_scale_exp(wave_max(amax));
    const float up = ldexpf(1.0f, sx), back = ldexpf(1.0f, -sx);
    const float4* pa = reinterpret_cast<const float4*>(dl + (size_t)(i0 + i) * npad + 8 * h);
    const float4* pb = reinterpret_cast<const float4*>(a + (size_t)(c0 + i) * npad + 8 * h);
    f32x16_t acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    double bs = 0.0;
    const int nks = (int)(npad / 16);                         // even: npad is a multiple of 32
    float4 av[2][2], bv[2][2];                                // two k-steps; the next pair is requested before this one is used
    auto fetch = [&](float4 (&a)[2][2], float4 (&b)[2][2], int s0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a[u][0] = pa[4 * (s0 + u)]; a[u][1] = pa[4 * (s0 + u) + 1];
            b[u][0] = pb[4 * (s0 + u)]; b[u][1] = pb[4 * (s0 + u) + 1];
        }
    };
    fetch(av, bv, 0);
    for (int s0 = 0; s0 < nks; s0 += 2) {
        float4 an[2][2], bn[2][2];
        fetch(an, bn, s0 + 2 < nks ? s0 + 2 : s0);            // clamped to the last pair
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x8_t va = {av[u][0].x, av[u][0].y, av[u][0].z, av[u][0].w, av[u][1].x, av[u][1].y, av[u][1].z, av[u][1].w};
            const f32x8_t vb = {bv[u][0].x, bv[u][0].y, bv[u][0].z, bv[u][0].w, bv[u][1].x, bv[u][1].y, bv[u][1].z, bv[u][1].w};
            half8_t ah, al, bh, bl;
            split16(va * up, ah, al);
            split16(vb, bh, bl);
            acc = mfma3(ah, al, bh, bl, acc);
            if (db) {                                         // wave-uniform
#pragma unroll
                for (int j = 0; j < 8; ++j) bs += (double)va[j];
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) { av[u][v] = an[u][v]; bv[u][v] = bn[u][v]; }
    }
    const int c = c0 + i;                                     // this lane's column
    if (c < ld) {
#pragma unroll
        for (int q = 0; q < 16; ++q) dW[(size_t)(i0 + (q & 3) + 8 * (q >> 2) + 4 * h) * ld + c] = acc[q] * back;
    }
    if (db) {
        bs += __shfl_xor(bs, 32, kWave);
        if (h == 0) db[i0 + i] = (float)bs;
    }
}

__global__ void __launch_bounds__(kGwBlock)
k_marl_critic_grad_weights(GradWArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int item = blockIdx.x * (kGwBlock / kWave) + wave, total = A.n_nets * A.per_net + 1;
    if (item >= total) return;                                // wave-uniform; no barrier in this kernel
    const long long npad = A.npad;
    if (item == total - 1) {                                  // d bq of every net and the loss
        double lsum = 0.0;
        for (int c = 0; c < A.n_nets; ++c) {
            const GradWNet& G = A.net[c];
            double se = 0.0, sl = 0.0;
            for (long long b = lane; b < npad; b += kWave) {
                const double dv = (double)G.diff[b];
                se += (double)G.e[b];
                sl += dv * dv;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                se += __shfl_xor(se, o, kWave);
                sl += __shfl_xor(sl, o, kWave);
            }
            if (lane == 0) G.dqb[0] = (float)se;
            lsum += sl;
        }
        if (lane == 0) A.loss[0] = (float)(lsum / (double)A.n_rows);
        return;
    }
    const int c = item / A.per_net;
    int k = item % A.per_net;
    const GradWNet& G = A.net[c];
    const int nt = A.ntiles;
    if (k < A.t1) {
        const int it = k / A.c1, ct = k % A.c1;
        grad_w_tile(G.d1, A.x, G.tmax, nt, npad, 32 * it, 32 * ct, G.dW1, A.IN, ct == 0 ? G.db1 : nullptr, lane);
        return;
    }
    k -= A.t1;
    if (k < A.t2) {
        const int cts = A.F1 / 32, it = k / cts, ct = k % cts;
        grad_w_tile(G.d2, G.h1, G.tmax + nt, nt, npad, 32 * it, 32 * ct, G.dW2, A.F1, ct == 0 ? G.db2 : nullptr, lane);
        return;
    }
    k -= A.t2;
    if (k < A.t3) {
        const int cts = A.F2 / 32, it = k / cts, ct = k % cts;
        grad_w_tile(G.d3, G.h2, G.tmax + 2 * nt, nt, npad, 32 * it, 32 * ct, G.dW3, A.F2, ct == 0 ? G.db3 : nullptr, lane);
        return;
    }
    k -= A.t3;
    {   // d wq: 8 features per wavefront, 8 lanes per feature; lane (f, c) adds the float4 blocks c, c + 8, .. of the batch in
        // ascending order, then the 8 partial sums meet in a fixed butterfly
        const int f = kGwFeat * k + (lane >> 3), c8 = lane & 7;
        const float4* ph = reinterpret_cast<const float4*>(G.h3 + (size_t)f * npad);
        const float4* pe = reinterpret_cast<const float4*>(G.e);
        double s = 0.0;
        for (long long b = c8; b < npad / 4; b += 8) {        // npad / 4 is a multiple of 8
            const float4 hv = ph[b], ev = pe[b];
            s += (double)ev.x * (double)hv.x;
            s += (double)ev.y * (double)hv.y;
            s += (double)ev.z * (double)hv.z;
            s += (double)ev.w * (double)hv.w;
        }
#pragma unroll
        for (int o = 1; o <= 4; o <<= 1) s += __shfl_xor(s, o, kWave);
        if (c8 == 0) G.dqw[f] = (float)s;
    }
}

inline long long round32(long long v) { return (v + 31) / 32 * 32; }

// floats of the tiles' maxima of one net, kept a multiple of 4 so that what follows stays on 16 bytes
inline long long tmax_floats(long long ntiles) { return (3 * ntiles + 3) / 4 * 4; }

inline long long net_floats(long long npad, int F1, int F2, int F3) {
    return 2 * (long long)(F1 + F2 + F3) * npad + 2 * npad + tmax_floats(npad / 32);
}

}  // namespace

bool marl_critic_grad_supported(int S, int A, int F1, int F2, int F3) { return marl_critic_supported(S, A, F1, F2, F3); }

size_t marl_critic_grad_workspace(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets) {
    if (n_rows < 1 || n_nets < 1 || n_nets > 2 || !marl_critic_grad_supported(S, A, F1, F2, F3)) return 0;
    const long long npad = round32(n_rows);
    return (size_t)(round32(S + A) * npad + n_nets * net_floats(npad, F1, F2, F3)) * sizeof(float);
}

hipError_t launch_marl_critic_grad(long long n_rows, int S, int A, int F1, int F2, int F3, int n_nets, const RisVecMarlCriticGradNet* nets,
                                   const RisVecMarlCriticGrads* grads, const float* state, const float* action, const float* target,
                                   float* q1, float* q2, float* loss, void* workspace, hipStream_t st) {
    if (!marl_critic_grad_supported(S, A, F1, F2, F3) || n_nets < 1 || n_nets > 2 || n_rows < 1) return hipErrorInvalidValue;
    const long long npad = round32(n_rows), ntiles = npad / 32;
    const int XF = (int)round32(S + A), MT2 = F2 / 128, MT3 = F3 / 128;
    GradRowArgs r{};
    r.n_rows = (int)n_rows; r.S = S; r.NA = A; r.KS = ks_of(S + A); r.NG = F1 / 32; r.F1 = F1; r.F2 = F2; r.F3 = F3; r.XF = XF;
    r.npad = npad; r.state = state; r.action = action; r.target = target;
    GradWArgs w{};
    w.n_rows = (int)n_rows; w.n_nets = n_nets; w.IN = S + A; w.F1 = F1; w.F2 = F2; w.F3 = F3; w.ntiles = (int)ntiles;
    w.c1 = XF / 32; w.t1 = (F1 / 32) * w.c1; w.t2 = (F2 / 32) * (F1 / 32); w.t3 = (F3 / 32) * (F2 / 32); w.tq = F3 / kGwFeat;
    w.per_net = w.t1 + w.t2 + w.t3 + w.tq; w.npad = npad; w.loss = loss;
    float* p = static_cast<float*>(workspace);
    r.x = p; w.x = p;
    p += (size_t)XF * npad;
    for (int c = 0; c < 2; ++c) {
        const int k = c < n_nets ? c : 0;                     // a single net fills both slots
        GradNetPtrs& g = r.net[c];
        float* b = p + (size_t)k * net_floats(npad, F1, F2, F3);
        g.fwd = marl_net_ptrs(nets[k].fwd); g.W2 = nets[k].W2; g.W3 = nets[k].W3;
        g.h1 = b; b += (size_t)F1 * npad; g.h2 = b; b += (size_t)F2 * npad; g.h3 = b; b += (size_t)F3 * npad;
        g.d1 = b; b += (size_t)F1 * npad; g.d2 = b; b += (size_t)F2 * npad; g.d3 = b; b += (size_t)F3 * npad;
        g.e = b; b += npad; g.diff = b; b += npad; g.tmax = b;
        g.q = k == 0 ? q1 : q2;
        const RisVecMarlCriticGrads& o = grads[k];
        w.net[c] = GradWNet{g.h1, g.h2, g.h3, g.d1, g.d2, g.d3, g.e, g.diff, g.tmax, o.dW1, o.db1, o.dW2, o.db2, o.dW3, o.db3, o.dqw, o.dqb};
    }
    note_kernel("k_marl_critic_grad_rows<%d,%d>x%d -> k_marl_critic_grad_weights", MT2, MT3, n_nets);
    const size_t lds = (size_t)(r.KS + std::max(2 * r.NG, 8 * MT2 + 8 * MT3)) * 2 * kWave * sizeof(uint4) +
                       (size_t)kRedSlots * kCriticWaves * 32 * sizeof(float);
    hipError_t err = dispatch_mt2_mt3(F2, F3, [&](auto mt2, auto mt3) {
        return launch_dynamic_lds(k_marl_critic_grad_rows<decltype(mt2)::value, decltype(mt3)::value>, dim3((unsigned)ntiles, (unsigned)n_nets),
                                  dim3(kMcBlock), lds, st, r);
    });
    if (err != hipSuccess) return err;
    const int items = n_nets * w.per_net + 1, per_block = kGwBlock / kWave;
    hipLaunchKernelGGL(k_marl_critic_grad_weights, dim3((unsigned)((items + per_block - 1) / per_block)), dim3(kGwBlock), 0, st, w);
    return hipGetLastError();
}

}  // namespace risvec
